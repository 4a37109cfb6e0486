"""A block of confidential transfers executed in one call (zk_confidential_block_execute) against a sequential Python model
of the seven steps include/zkamd.h states, over oracle/jubjub.py; and zk_g_epoch against the oracle's group hash.  Proofs are
forged for chosen public inputs with the trapdoor of a small key (xt_verify_cases.trapdoor_proof), signatures come from
redjubjub_cases.sign.  Every function takes `lib` (a ZkLib over one build of the C ABI)."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

import zero_chain_amd as zk
from zero_chain_amd import _lib as zl
from oracle import jubjub as jj
import helpers
import redjubjub_cases as rc
import xt_verify_cases as xc

DUE, ROLLED = zk.BLOCK_ROLLOVER_DUE, zk.BLOCK_ROLLED
IDENTITY = xc.enc_y(1)
ZERO_CT = (IDENTITY, IDENTITY)
FIELDS = zk.CONFIDENTIAL_XT_POINTS
# the encodings of an extrinsic that the call decodes, and the field each is in zk_confidential_verify_batch's push order
XT_POINTS = ("enc_key_sender", "enc_key_recipient", "left_amount_sender", "left_amount_recipient", "right_randomness", "left_fee", "rvk", "nonce")


# ---------------------------------------------------------------------------------------------- points
_KNOWN = {}     # encoding -> (status, x, y) of the points made here: multiples of the generator, so of prime order by construction
_STREAM = []


def point(k):
    """the k-th point of one stream of distinct prime-order points (a start point plus k times the generator); its encoding"""
    g = jj.note_commitment_randomness_generator()
    while len(_STREAM) <= k:
        _STREAM.append(jj.add(_STREAM[-1], g) if _STREAM else xc.prime_order_points()[0])
        _KNOWN[jj.write_point(_STREAM[-1])] = (0,) + _STREAM[-1]
    return jj.write_point(_STREAM[k])


def decode(enc):
    """(status, x, y) as IntoXY judges the encoding"""
    enc = bytes(enc)
    if enc not in _KNOWN:
        st, xy = xc.expected(enc)
        _KNOWN[enc] = (st, int.from_bytes(xy[:32], "little"), int.from_bytes(xy[32:], "little"))
    return _KNOWN[enc]


def read_ct(ct):
    """Ciphertext::read: the two points, or None"""
    l, r = decode(ct[0]), decode(ct[1])
    return None if l[0] or r[0] else [l[1:], r[1:]]


def neg(p):
    return (-p[0] % jj.R, p[1])


@functools.lru_cache(maxsize=None)
def keypair(j):
    sk = 0x1234567 + 977 * j
    return sk, jj.write_point(jj.mul(rc.generator(), sk))


@functools.lru_cache(maxsize=None)
def sig_reason(vk, sig, msg):
    return rc.verify(vk, sig, msg)


@functools.lru_cache(maxsize=None)
def forged(inputs):
    return xc.trapdoor_proof(xc.small_conf_key()[0], list(inputs))


# ---------------------------------------------------------------------------------------------- the model
class Model:
    """encrypted_balances::confidential_transfer, one extrinsic after another"""

    def __init__(self, accounts, pool, g_epoch):
        self.index = {bytes(a["enc_key"]): k for k, a in enumerate(accounts)}
        assert len(self.index) == len(accounts)
        self.acc = []
        for a in accounts:
            bal, pen = read_ct(a.get("balance") or ZERO_CT), read_ct(a.get("pending") or ZERO_CT)
            self.acc.append(dict(src=a, bal=bal, pen=pen, bad=bal is None or pen is None, due=bool(a.get("flags", 0) & DUE), rolled=False, named=False))
        self.pool = [bytes(x) for x in pool]
        self.g_epoch = bytes(g_epoch)
        self.verdicts = []

    def balance_met(self, sender, recipient):
        """the sender's balance after the two rollovers of step 3, nothing changed"""
        s = self.acc[self.index[bytes(sender)]]
        if s["due"] and not s["rolled"]:
            return [jj.add(s["bal"][c], s["pen"][c]) for c in range(2)]
        return list(s["bal"])

    def inputs(self, x, balance):
        """the 22 public inputs, or the refusal (field name, reason)"""
        out = []
        for k, name in enumerate(FIELDS):
            if k in (6, 7):
                out += list(balance[k - 6])
                continue
            st, px, py = decode(self.g_epoch if name == "g_epoch" else x[name])
            if st:
                return None, (name, zk.INTO_XY_REASONS[st])
            out += [px, py]
        return tuple(out), None

    def step(self, x, sig=None, msg=None):
        v = self._step(x, sig, msg)
        self.verdicts.append(v)
        return v

    def _step(self, x, sig, msg):
        if sig is not None:
            why = sig_reason(bytes(x["rvk"]), bytes(sig), bytes(msg))
            if why:
                return ("bad signature", zk.REDJUBJUB_REASONS[why])
        s, r = self.acc[self.index[bytes(x["enc_key_sender"])]], self.acc[self.index[bytes(x["enc_key_recipient"])]]
        s["named"] = r["named"] = True
        if s["bad"] or r["bad"]:
            return ("bad account", None)
        for a in (s, r):
            if a["due"] and not a["rolled"]:
                a["bal"] = [jj.add(a["bal"][c], a["pen"][c]) for c in range(2)]
                a["pen"] = [jj.ZERO, jj.ZERO]
                a["rolled"] = True
        if bytes(x["nonce"]) in self.pool:
            return ("nonce used", None)
        inputs, refusal = self.inputs(x, s["bal"])
        if refusal:
            return ("refused point", refusal)
        if bytes(x["proof"]) != forged(inputs):
            return ("invalid proof", None)
        self.pool.append(bytes(x["nonce"]))
        rand = decode(x["right_randomness"])[1:]
        for name in ("left_amount_sender", "left_fee"):
            s["bal"] = [jj.add(s["bal"][0], neg(decode(x[name])[1:])), jj.add(s["bal"][1], neg(rand))]
        r["pen"] = [jj.add(r["pen"][0], decode(x["left_amount_recipient"])[1:]), jj.add(r["pen"][1], rand)]
        return ("accepted", None)

    def accounts_out(self):
        out = []
        for a in self.acc:
            src = a["src"]
            o = dict(enc_key=bytes(src["enc_key"]), flags=int(src.get("flags", 0)))
            if not a["named"]:
                o["balance"], o["pending"] = tuple(src.get("balance") or ZERO_CT), tuple(src.get("pending") or ZERO_CT)
            elif a["bad"]:
                o["balance"] = o["pending"] = (bytes(32), bytes(32))
            else:
                o["balance"], o["pending"] = tuple(jj.write_point(p) for p in a["bal"]), tuple(jj.write_point(p) for p in a["pen"])
                if a["rolled"]:
                    o["flags"] |= ROLLED
            out.append(o)
        return out


# ---------------------------------------------------------------------------------------------- building a block
class Block:
    """A block under construction.  add() forges the proof against the balance the model says the extrinsic meets ("valid"),
    against the balance as if nothing before it in the block had been accepted ("unmoved"), or spoils it ("bad")."""

    def __init__(self, accounts, pool=(), g_epoch=None, signed=True, first_point=0):
        self.accounts, self.pool, self.signed = list(accounts), [bytes(x) for x in pool], signed
        self.g_epoch = bytes(g_epoch) if g_epoch is not None else jj.write_point(jj.find_group_hash((0).to_bytes(4, "little"), b"zcgepoch"))
        self.xts, self.sigs, self.msgs = [], [], []
        self.live = Model(self.accounts, self.pool, self.g_epoch)
        self.unmoved = Model(self.accounts, self.pool, self.g_epoch)
        self.next_point = first_point
        self.expect = {}

    def fresh(self):
        self.next_point += 1
        return point(self.next_point - 1)

    def add(self, sender, recipient, proof="valid", sig="good", nonce=None, **fields):
        i = len(self.xts)
        sk, rvk = keypair(i % 3)
        x = dict(enc_key_sender=bytes(sender), enc_key_recipient=bytes(recipient), left_amount_sender=self.fresh(), left_amount_recipient=self.fresh(),
                 left_fee=self.fresh(), right_randomness=self.fresh(), rvk=rvk if self.signed else self.fresh(), nonce=bytes(nonce) if nonce else self.fresh(),
                 rsk=bytes(32), enc_balance=bytes(64))
        x.update({k: bytes(v) for k, v in fields.items()})
        msg = b"extrinsic %d of the block" % i + bytes(i % 7)
        sg = None
        if self.signed:
            sg = rc.sign(sk, bytes([i % 256]) * 80, msg)
            if sig == "bad":
                sg = sg[:32] + ((int.from_bytes(sg[32:], "little") + 1) % rc.S).to_bytes(32, "little")
            elif sig == "bad R":
                sg = xc.enc_y(2) + sg[32:]
        src = self.unmoved if proof == "unmoved" else self.live
        s = src.acc[src.index[x["enc_key_sender"]]]
        r = src.acc[src.index[x["enc_key_recipient"]]]
        x["proof"] = xc.good_conf(0)[1]   # (a well-formed proof of something else)
        if not (s["bad"] or r["bad"]):
            inputs, refusal = src.inputs(x, src.balance_met(sender, recipient))
            if inputs is not None:
                x["proof"] = forged(inputs)
                if proof == "bad":
                    spoiled = bytearray(x["proof"])
                    spoiled[150] ^= 1
                    x["proof"] = bytes(spoiled)
        self.live.step(x, sg, msg)
        self.xts.append(x)
        self.sigs.append(sg)
        self.msgs.append(msg)
        return i

    def args(self):
        return self.xts, self.accounts, self.pool, self.g_epoch, (self.sigs if self.signed else None), (self.msgs if self.signed else None)

    def want(self):
        m = Model(self.accounts, self.pool, self.g_epoch)
        for x, sg, msg in zip(self.xts, self.sigs, self.msgs):
            m.step(x, sg, msg)
        return m.verdicts, m.accounts_out()

    def distinct(self):
        pts = {x[f] for x in self.xts for f in XT_POINTS} | {self.g_epoch}
        for a in self.accounts:
            pts |= set(a.get("balance") or ZERO_CT) | set(a.get("pending") or ZERO_CT)
        return len(pts)


def account(k, flags=0, pending=True):
    """account k: its key and ciphertexts are points 1000 + 8 k .. of the stream"""
    b = 1000 + 8 * k
    return dict(enc_key=point(b), balance=(point(b + 1), point(b + 2)), pending=(point(b + 3), point(b + 4)) if pending else None, flags=flags)


UNDECODABLE = xc.enc_y(2)


def torsion():
    return jj.write_point(jj.add(xc.prime_order_points()[0], xc.torsion_points()[2]))


def _honest(signed=True):
    a = [account(0, DUE), account(1), account(2, DUE, pending=False), account(3, DUE), account(4, DUE)]   # 4: named by nobody
    a[4]["balance"] = (xc.enc_y(1, 1), point(1037))   # x = 0 with the sign bit set: copied through as it came
    b = Block(a, signed=signed)
    b.add(a[0]["enc_key"], a[2]["enc_key"])
    b.add(a[1]["enc_key"], a[2]["enc_key"])   # a shared recipient; the sender is not due
    b.add(a[3]["enc_key"], a[3]["enc_key"])   # to oneself
    b.add(a[2]["enc_key"], a[0]["enc_key"])
    b.expect = dict(verdicts=["accepted"] * 4, rounds=1, proofs_verified=4)
    return b


def _one_sender_twice(second):
    a = [account(k, DUE if k % 2 else 0) for k in range(5)]
    b = Block(a)
    b.add(a[0]["enc_key"], a[1]["enc_key"])
    b.add(a[0]["enc_key"], a[2]["enc_key"], proof=second)
    b.add(a[3]["enc_key"], a[1]["enc_key"])
    b.add(a[4]["enc_key"], a[0]["enc_key"])
    # round 1 verifies all four, and the second waits: its sender's balance moved.  Round 2 verifies it alone.
    b.expect = dict(verdicts=["accepted", "accepted" if second == "valid" else "invalid proof", "accepted", "accepted"], rounds=2, proofs_verified=5)
    return b


def _first_rejected(how):
    a = [account(k, DUE if k % 2 == 0 else 0) for k in range(4)]
    b = Block(a)
    if how == "proof":
        b.add(a[0]["enc_key"], a[1]["enc_key"], proof="bad")
    else:
        b.add(a[0]["enc_key"], a[1]["enc_key"], sig="bad")
    b.add(a[0]["enc_key"], a[2]["enc_key"], proof="unmoved")
    b.add(a[1]["enc_key"], a[3]["enc_key"])
    b.add(a[3]["enc_key"], a[0]["enc_key"])
    b.expect = dict(verdicts=["invalid proof" if how == "proof" else "bad signature", "accepted", "accepted", "accepted"], rounds=1,
                    proofs_verified=4 if how == "proof" else 3)
    return b


def _same_nonce(first_accepted):
    a = [account(k) for k in range(4)]
    b = Block(a, pool=[point(2900)])
    n = point(2901)
    b.add(a[0]["enc_key"], a[1]["enc_key"], nonce=n, proof="valid" if first_accepted else "bad")
    b.add(a[2]["enc_key"], a[3]["enc_key"], nonce=n)
    b.add(a[1]["enc_key"], a[0]["enc_key"], nonce=point(2900))   # a nonce the pool came with
    b.add(a[3]["enc_key"], a[2]["enc_key"])
    # the second shares no sender with the first, so one round settles it either way: by the pool as the sweep has grown it
    b.expect = dict(verdicts=["accepted", "nonce used", "nonce used", "accepted"] if first_accepted else ["invalid proof", "accepted", "nonce used", "accepted"],
                    rounds=1, proofs_verified=3)
    return b


def _due_account_named_once(how):
    a = [account(0, DUE), account(1), account(2), account(3, DUE)]
    b = Block(a)
    if how == "signature":
        b.add(a[0]["enc_key"], a[1]["enc_key"], sig="bad R")
    else:
        b.add(a[0]["enc_key"], a[1]["enc_key"], proof="bad")
    b.add(a[1]["enc_key"], a[2]["enc_key"])
    b.add(a[2]["enc_key"], a[3]["enc_key"])
    b.add(a[3]["enc_key"], a[1]["enc_key"])
    b.expect = dict(verdicts=["bad signature" if how == "signature" else "invalid proof"] + ["accepted"] * 3, rounds=1,
                    proofs_verified=3 if how == "signature" else 4, rolled_0=how != "signature")
    return b


def _refused_fields(bad):
    """every point of an extrinsic refused once.  Fields 1 and 2 need an account under that key; fields 7 and 8 are the stored
    balance, which step 2 judges before step 5 can: BAD_ACCOUNT."""
    a = [account(k, DUE if k % 3 == 0 else 0) for k in range(10)]
    a.append(dict(enc_key=bad, balance=a[0]["balance"], pending=None, flags=0))
    a[6]["balance"] = (bad, a[6]["balance"][1])
    a[7]["balance"] = (a[7]["balance"][0], bad)
    b = Block(a)
    rcp = a[9]["enc_key"]
    b.add(bad, rcp)                                            # field 1
    b.add(a[0]["enc_key"], bad)                                # field 2
    b.add(a[1]["enc_key"], rcp, left_amount_sender=bad)        # 3
    b.add(a[2]["enc_key"], rcp, left_amount_recipient=bad)     # 4
    b.add(a[3]["enc_key"], rcp, right_randomness=bad)          # 5
    b.add(a[4]["enc_key"], rcp, left_fee=bad)                  # 6
    b.add(a[6]["enc_key"], rcp)                                # 7: the balance's left
    b.add(a[7]["enc_key"], rcp)                                # 8: the balance's right
    b.add(a[5]["enc_key"], rcp, nonce=bad)                     # 11
    b.add(a[8]["enc_key"], rcp)
    b.add(a[9]["enc_key"], a[8]["enc_key"], left_fee=bad, right_randomness=bad)   # two refused: the first in push order, 5
    st = decode(bad)[0]
    assert st in (2, 3)
    why = zk.INTO_XY_REASONS[st]
    ref = lambda k: ("refused point", (FIELDS[k - 1], why))
    b.expect = dict(verdicts=[ref(1), ref(2), ref(3), ref(4), ref(5), ref(6), ("bad account", None), ("bad account", None), ref(11), ("accepted", None),
                              ref(5)], rounds=1, proofs_verified=1)
    return b


def _refused_rvk_and_epoch(bad):
    a = [account(k) for k in range(4)]
    b = Block(a, signed=False, pool=[point(2900)])
    b.add(a[0]["enc_key"], a[1]["enc_key"], rvk=bad)           # field 9 (unsigned: with signatures a bad rvk is a bad signature)
    e = Block(a, signed=False, pool=[point(2900)], g_epoch=bad)
    e.add(a[0]["enc_key"], a[1]["enc_key"])                          # field 10
    e.add(a[1]["enc_key"], a[2]["enc_key"], left_amount_sender=bad)  # field 3 comes first
    e.add(a[2]["enc_key"], a[3]["enc_key"], nonce=point(2900))       # step 4 comes before step 5
    e.add(a[3]["enc_key"], a[0]["enc_key"], nonce=bad)               # field 10 before 11
    why = zk.INTO_XY_REASONS[decode(bad)[0]]
    b.expect = dict(verdicts=[("refused point", ("rvk", why))], rounds=1, proofs_verified=0)
    e.expect = dict(verdicts=[("refused point", ("g_epoch", why)), ("refused point", ("left_amount_sender", why)), ("nonce used", None),
                              ("refused point", ("g_epoch", why))], rounds=1, proofs_verified=0)
    return b, e


def _bad_accounts():
    a = [account(k, DUE) for k in range(6)]
    a[1]["balance"] = (UNDECODABLE, a[1]["balance"][1])
    a[2]["pending"] = (a[2]["pending"][0], torsion())
    a[5]["pending"] = (torsion(), a[5]["pending"][1])   # named by nobody: copied through
    b = Block(a)
    b.add(a[1]["enc_key"], a[0]["enc_key"])   # the sender's balance; account 0 is due, and is not rolled over by this one
    b.add(a[3]["enc_key"], a[2]["enc_key"])   # the recipient's pending; 3 likewise
    b.add(a[4]["enc_key"], a[4]["enc_key"])
    b.add(a[0]["enc_key"], a[4]["enc_key"])   # ... but 0 is by this one
    b.expect = dict(verdicts=["bad account", "bad account", "accepted", "accepted"], rounds=1, proofs_verified=2)
    return b


@functools.lru_cache(maxsize=None)
def cases():
    und = _refused_rvk_and_epoch(UNDECODABLE)
    tor = _refused_rvk_and_epoch(torsion())
    return {
        "honest": _honest(),
        "honest_unsigned": _honest(signed=False),
        "one_sender_twice_both_valid": _one_sender_twice("valid"),
        "one_sender_twice_second_against_the_stored_balance": _one_sender_twice("unmoved"),
        "first_of_a_sender_bad_proof": _first_rejected("proof"),
        "first_of_a_sender_bad_signature": _first_rejected("signature"),
        "same_nonce_first_accepted": _same_nonce(True),
        "same_nonce_first_rejected": _same_nonce(False),
        "due_account_named_by_a_bad_signature_only": _due_account_named_once("signature"),
        "due_account_named_by_an_invalid_proof_only": _due_account_named_once("proof"),
        "refused_fields_undecodable": _refused_fields(UNDECODABLE),
        "refused_fields_torsion": _refused_fields(torsion()),
        "refused_rvk_undecodable": und[0],
        "refused_g_epoch_undecodable": und[1],
        "refused_rvk_torsion": tor[0],
        "refused_g_epoch_torsion": tor[1],
        "unreadable_accounts": _bad_accounts(),
    }


CASE_NAMES = ("honest", "honest_unsigned", "one_sender_twice_both_valid", "one_sender_twice_second_against_the_stored_balance",
              "first_of_a_sender_bad_proof", "first_of_a_sender_bad_signature", "same_nonce_first_accepted", "same_nonce_first_rejected",
              "due_account_named_by_a_bad_signature_only", "due_account_named_by_an_invalid_proof_only", "refused_fields_undecodable",
              "refused_fields_torsion", "refused_rvk_undecodable", "refused_g_epoch_undecodable", "refused_rvk_torsion", "refused_g_epoch_torsion",
              "unreadable_accounts")


# ---------------------------------------------------------------------------------------------- running
@functools.lru_cache(maxsize=None)
def _vk_bytes():
    return xc.small_conf_key()[1]


def execute(lib, block):
    pvk = zk.prepare_verifying_key(_vk_bytes(), lib=lib)
    try:
        return zk.execute_confidential_block(pvk, *block.args())
    finally:
        pvk.close()


def check(block, got):
    """verdicts, accounts and counters of one call against the model and the case's own statement"""
    verdicts, accounts, stats = got
    want_v, want_a = block.want()
    for i, (g, w) in enumerate(zip(verdicts, want_v)):
        assert g == w, "extrinsic %d: %r, the model says %r" % (i, g, w)
    assert len(verdicts) == len(want_v)
    for k, (g, w) in enumerate(zip(accounts, want_a)):
        assert g == w, "account %d: %r, the model says %r" % (k, g, w)
    assert len(accounts) == len(want_a)
    assert stats["points_decoded"] == block.distinct()
    ex = block.expect
    if "verdicts" in ex:   # what the case was built to show, stated without the model
        assert [v if isinstance(w, tuple) else v[0] for v, w in zip(verdicts, ex["verdicts"])] == list(ex["verdicts"])
    for k in ("rounds", "proofs_verified"):
        if k in ex:
            assert stats[k] == ex[k], (k, stats)
    if "rolled_0" in ex:
        assert bool(accounts[0]["flags"] & ROLLED) == ex["rolled_0"]
        if not ex["rolled_0"]:
            assert accounts[0] == dict(block.accounts[0], enc_key=bytes(block.accounts[0]["enc_key"]))


def run_case(lib, name):
    block = cases()[name]
    check(block, execute(lib, block))


def _raw(lib, pvk, block, n=None, null=(), n_accounts=None):
    """the entry through the ctypes handle, every output pre-filled with 0xAA: (status, accounts bytes, verdict bytes, stats bytes)"""
    xts, accounts, pool, ge, sigs, msgs = block.args()
    n = len(xts) if n is None else n
    na = len(accounts) if n_accounts is None else n_accounts
    arr = (zl.ConfidentialXt * max(len(xts), 1))()
    for dst, x in zip(arr, xts):
        for f in zk.XT_FIELDS:
            getattr(dst, f)[:] = x[f]
    acc = (zl.BlockAccount * max(len(accounts), 1))()
    for dst, a in zip(acc, accounts):
        dst.enc_key[:] = a["enc_key"]
        dst.balance[:] = b"".join(a.get("balance") or ZERO_CT)
        dst.pending[:] = b"".join(a.get("pending") or ZERO_CT)
        dst.flags = a.get("flags", 0)
    fill = lambda size: np.full(max(size, 1), 0xAA, dtype=np.uint8)
    out, ver, st = fill(C.sizeof(zl.BlockAccount) * len(accounts)), fill(4 * len(xts)), fill(16)
    pb = np.frombuffer(b"".join(pool) or b"\0", dtype=np.uint8).copy()
    gb = np.frombuffer(ge, dtype=np.uint8).copy()
    sb = np.frombuffer(b"".join(sigs), dtype=np.uint8).copy() if sigs else None
    mb = np.frombuffer(b"".join(msgs), dtype=np.uint8).copy() if msgs else None
    offs = np.zeros(len(xts) + 1, dtype=np.uint64)
    if msgs:
        offs[1:] = np.cumsum([len(m) for m in msgs])
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    arg = dict(xts=arr, sigs=None if sb is None else ptr(sb), msgs=None if mb is None else ptr(mb), offs=ptr(offs), accounts=acc, pool=ptr(pb) if pool else None,
               g_epoch=ptr(gb), out=C.cast(ptr(out), C.POINTER(zl.BlockAccount)), verdicts=C.cast(ptr(ver), C.POINTER(zl.BlockVerdict)),
               stats=C.cast(ptr(st), C.POINTER(zl.BlockStats)))
    for k in null:
        arg[k] = None
    status = lib.zk_confidential_block_execute(pvk._h, n, arg["xts"], arg["sigs"], arg["msgs"], arg["offs"], na, arg["accounts"], len(pool), arg["pool"],
                                               arg["g_epoch"], arg["out"], arg["verdicts"], arg["stats"])
    return status, out.tobytes(), ver.tobytes(), st.tobytes()


class _OtherAccounts:
    """the extrinsics of a block over other accounts"""

    def __init__(self, block, accounts):
        self.block, self.accounts = block, accounts

    def args(self):
        return (self.block.xts, self.accounts) + self.block.args()[2:]


def bad_arguments(lib):
    """the caller's own mistakes: ZK_ERR_INVALID_ARGUMENT, the index in the text, nothing written"""
    pvk = zk.prepare_verifying_key(_vk_bytes(), lib=lib)
    try:
        honest = cases()["honest"]
        untouched = lambda r: all(set(b) <= {0xAA} for b in r[1:])
        # a key that is not among the accounts (the recipient of extrinsic 3 is account 0)
        short = _OtherAccounts(honest, honest.accounts[1:])
        r = _raw(lib, pvk, short)
        assert r[0] == 16 and untouched(r) and b"extrinsic 0" in lib.zk_last_error()   # (its sender is account 0 too)
        # two accounts with equal keys
        twice = _OtherAccounts(honest, honest.accounts + [dict(honest.accounts[2], balance=None)])
        r = _raw(lib, pvk, twice)
        assert r[0] == 16 and untouched(r) and b"account 5" in lib.zk_last_error()
        # NULL buffers with non-zero counts
        for null in (("xts",), ("verdicts",), ("g_epoch",), ("accounts",), ("out",), ("pool",), ("offs",)):
            blk = cases()["same_nonce_first_accepted"] if null == ("pool",) else honest
            r = _raw(lib, pvk, blk, null=null)
            assert r[0] == 16 and untouched(r), null
        assert _raw(lib, pvk, honest, null=("stats",))[0] == 0   # stats_out may be NULL
        # nothing to do: the accounts are copied through, flags and all, and no verdict is written
        r = _raw(lib, pvk, honest, n=0)
        acc = (zl.BlockAccount * len(honest.accounts)).from_buffer_copy(r[1])
        assert r[0] == 0 and set(r[2]) == {0xAA} and r[3] == bytes(16)
        for o, a in zip(acc, honest.accounts):
            assert bytes(o.enc_key) == a["enc_key"] and bytes(o.balance) == b"".join(a.get("balance") or ZERO_CT) and o.flags == a["flags"]
            assert bytes(o.pending) == b"".join(a.get("pending") or ZERO_CT)
        assert _raw(lib, pvk, honest, n=0, null=("xts", "verdicts", "g_epoch", "sigs", "msgs", "offs"))[0] == 0
        assert zk.execute_confidential_block(pvk, [], [], [], honest.g_epoch) == ([], [], dict(rounds=0, proofs_verified=0, points_decoded=0))
    finally:
        pvk.close()
    # a key with three inputs
    r1, asg, P3, pk3 = helpers.small_case(1, 4, 6, 9)
    pvk3 = zk.prepare_verifying_key(xc.vk_bytes_of(pk3), lib=lib)
    try:
        with pytest.raises(zk.ZkError) as e:
            zk.execute_confidential_block(pvk3, *honest.args())
        assert e.value.variant == "MalformedVerifyingKey"
    finally:
        pvk3.close()


def g_epochs(lib):
    """zk_g_epoch against the oracle's find_group_hash, and epoch 0 against the reference's own vector"""
    for epoch in (0, 1, 2, 2 ** 32 - 1):
        want = jj.write_point(jj.find_group_hash(epoch.to_bytes(4, "little"), b"zcgepoch"))
        assert zk.g_epoch(epoch, lib=lib) == want, epoch
        assert decode(want)[0] == 0
    with open(os.path.join(helpers.GOLDEN, "zk_system_vectors.json")) as f:
        golden = json.load(f)["test_call_with_wrong_proof"]["g_epoch"]
    assert zk.g_epoch(0, lib=lib).hex() == golden and golden.startswith("0953f473") and golden.endswith("665a")
    assert lib.zk_g_epoch(7, None) == 16


# ---------------------------------------------------------------------------------------------- the shapes of the device form
@functools.lru_cache(maxsize=None)
def all_accepted(n):
    """n extrinsics of n senders to one recipient, all accepted: 2 n lanes of k_block_balance_xy"""
    a = [account(20 + k, DUE if k % 2 else 0) for k in range(n + 1)]
    b = Block(a, signed=False, first_point=3000)
    for k in range(n):
        b.add(a[k]["enc_key"], a[n]["enc_key"])
    b.expect = dict(verdicts=["accepted"] * n, rounds=1, proofs_verified=n)
    return b


@functools.lru_cache(maxsize=None)
def large_block():
    """130 extrinsics over 40 accounts, ten rejected for mixed reasons: more than 256 ops, so the scan crosses a workgroup, slots
    straddle the boundary and take the carry; every sender has three or four extrinsics, so the block takes several rounds"""
    a = [account(100 + k, DUE if k % 3 else 0) for k in range(40)]
    b = Block(a, pool=[point(2900)], first_point=5000)
    rejected = {7: dict(proof="bad"), 19: dict(sig="bad"), 33: dict(nonce=point(2900)), 41: dict(left_fee=UNDECODABLE), 58: dict(proof="unmoved"),
                64: dict(sig="bad R"), 77: dict(proof="bad"), 90: dict(right_randomness=torsion()), 101: dict(proof="bad"), 129: dict(sig="bad")}
    for i in range(130):
        b.add(a[i % 40]["enc_key"], a[(7 * i + 3) % 40]["enc_key"], **rejected.get(i, {}))
    got = [v[0] for v in b.live.verdicts]
    assert [i for i in range(130) if got[i] != "accepted"] == sorted(rejected), got
    assert {got[i] for i in rejected} == {"invalid proof", "bad signature", "nonce used", "refused point"}
    return b
