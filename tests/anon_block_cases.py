"""A block of anonymous transfers executed in one call (zk_anonymous_block_execute) against a sequential Python model of the
seven steps include/zkamd.h states, over oracle/jubjub.py.  The points, keys, signatures and the IntoXY judgement are those of
block_cases; proofs are forged for chosen public inputs with the trapdoor of a small key with 104 inputs
(xt_verify_cases.trapdoor_proof over helpers.small_case(32, 105, 6, 30)).  Every function takes `lib` (a ZkLib over one build
of the C ABI)."""
import ctypes as C
import functools

import numpy as np
import pytest

import zero_chain_amd as zk
from zero_chain_amd import _lib as zl
from oracle import jubjub as jj
import helpers
import block_cases as bc
import redjubjub_cases as rc
import xt_verify_cases as xc

DUE, ROLLED = bc.DUE, bc.ROLLED
ZERO_CT = bc.ZERO_CT
FIELDS = zk.ANONYMOUS_XT_POINTS
RING = 12
point, decode, read_ct, account, keypair = bc.point, bc.decode, bc.read_ct, bc.account, bc.keypair
UNDECODABLE, torsion = bc.UNDECODABLE, bc.torsion


@functools.lru_cache(maxsize=None)
def small_anon_key():
    r1, asg, P, pk = helpers.small_case(32, 105, 6, 30)
    return P, xc.vk_bytes_of(pk)


@functools.lru_cache(maxsize=None)
def forged(inputs):
    return xc.trapdoor_proof(small_anon_key()[0], list(inputs))


@functools.lru_cache(maxsize=None)
def some_proof():
    """a well-formed proof of something else"""
    return forged(tuple(range(1, 105)))


def xt_encodings(x):
    """the 27 encodings of an extrinsic that the call decodes"""
    return list(x["enc_keys"]) + list(x["left_ciphertexts"]) + [x["right_ciphertext"], x["rvk"], x["nonce"]]


# ---------------------------------------------------------------------------------------------- the model
class Model:
    """anonymous_balances::anonymous_transfer, one extrinsic after another"""

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

    def members(self, x):
        return [self.acc[self.index[bytes(k)]] for k in x["enc_keys"]]

    def balances_met(self, x):
        """the members' balances after the rollovers of step 3, nothing changed"""
        out = []
        for a in self.members(x):
            out.append([jj.add(a["bal"][c], a["pen"][c]) for c in range(2)] if a["due"] and not a["rolled"] else list(a["bal"]))
        return out

    def inputs(self, x, balances):
        """the 104 public inputs, or the refusal (field name, reason)"""
        enc = list(x["enc_keys"]) + list(x["left_ciphertexts"]) + [None] * 24 + [x["right_ciphertext"], x["rvk"], self.g_epoch, x["nonce"]]
        out = []
        for k, name in enumerate(FIELDS):
            if 24 <= k < 48:
                out += list(balances[(k - 24) % RING][(k - 24) // RING])
                continue
            st, px, py = decode(enc[k])
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
            why = bc.sig_reason(bytes(x["rvk"]), bytes(sig), bytes(msg))
            if why:
                return ("bad signature", zk.REDJUBJUB_REASONS[why])
        ring = self.members(x)
        for a in ring:
            a["named"] = True
        if any(a["bad"] for a in ring):
            return ("bad account", None)
        for a in ring:
            if a["due"] and not a["rolled"]:
                a["bal"] = [jj.add(a["bal"][c], a["pen"][c]) for c in range(2)]
                a["pen"] = [jj.ZERO, jj.ZERO]
                a["rolled"] = True
        if bytes(x["nonce"]) in self.pool:
            return ("nonce used", None)
        inputs, refusal = self.inputs(x, [a["bal"] for a in ring])
        if refusal:
            return ("refused point", refusal)
        if bytes(x["proof"]) != forged(inputs):
            return ("invalid proof", None)
        self.pool.append(bytes(x["nonce"]))
        right = decode(x["right_ciphertext"])[1:]
        for a, left in zip(ring, x["left_ciphertexts"]):
            a["pen"] = [jj.add(a["pen"][0], decode(left)[1:]), jj.add(a["pen"][1], right)]
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
    """A block under construction.  add() forges the proof against the balances the model says the ring's members hold when the
    extrinsic reaches step 5 ("valid"), or spoils it ("bad")."""

    def __init__(self, accounts, pool=(), g_epoch=None, signed=True, first_point=7000):
        self.accounts, self.pool, self.signed = list(accounts), [bytes(x) for x in pool], signed
        self.g_epoch = bytes(g_epoch) if g_epoch is not None else jj.write_point(jj.find_group_hash((0).to_bytes(4, "little"), b"zcgepoch"))
        self.xts, self.sigs, self.msgs = [], [], []
        self.live = Model(self.accounts, self.pool, self.g_epoch)
        self.next_point = first_point
        self.expect = {}

    def fresh(self):
        self.next_point += 1
        return point(self.next_point - 1)

    def add(self, ring, proof="valid", sig="good", nonce=None, lefts=None, **fields):
        """ring: twelve account indices (or keys as bytes); lefts: {member: encoding} in place of fresh points"""
        i = len(self.xts)
        sk, rvk = keypair(i % 3)
        keys = [bytes(k) if isinstance(k, (bytes, bytearray)) else bytes(self.accounts[k]["enc_key"]) for k in ring]
        assert len(keys) == RING
        x = dict(enc_keys=keys, left_ciphertexts=[self.fresh() for _ in range(RING)], right_ciphertext=self.fresh(),
                 rvk=rvk if self.signed else self.fresh(), nonce=bytes(nonce) if nonce else self.fresh(), rsk=bytes(32))
        for k, v in (lefts or {}).items():
            x["left_ciphertexts"][k] = bytes(v)
        x.update({k: bytes(v) for k, v in fields.items()})
        msg = b"anonymous extrinsic %d of the block" % i + bytes(i % 5)
        sg = None
        if self.signed:
            sg = rc.sign(sk, bytes([(i + 100) % 256]) * 80, msg)
            if sig == "bad":
                sg = sg[:32] + ((int.from_bytes(sg[32:], "little") + 1) % rc.S).to_bytes(32, "little")
            elif sig == "bad R":
                sg = xc.enc_y(2) + sg[32:]
        x["proof"] = some_proof()
        if not any(a["bad"] for a in self.live.members(x)):
            inputs, refusal = self.live.inputs(x, self.live.balances_met(x))
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
        pts = {bytes(e) for x in self.xts for e in xt_encodings(x)} | {self.g_epoch}
        for a in self.accounts:
            pts |= set(a.get("balance") or ZERO_CT) | set(a.get("pending") or ZERO_CT)
        return len(pts)


def sum_ct(cts):
    """the canonical bytes of a sum of (left, right) encodings"""
    acc = [jj.ZERO, jj.ZERO]
    for ct in cts:
        acc = [jj.add(acc[c], decode(ct[c])[1:]) for c in range(2)]
    return tuple(jj.write_point(p) for p in acc)


def as_given(a):
    return dict(enc_key=bytes(a["enc_key"]), balance=tuple(a.get("balance") or ZERO_CT), pending=tuple(a.get("pending") or ZERO_CT), flags=int(a.get("flags", 0)))


def _honest(signed=True):
    a = [account(k, DUE if k in (0, 3, 5, 8, 13, 16) else 0, pending=k != 5) for k in range(17)]   # 5: due with no pending; 16: named by nobody
    a[16]["balance"] = (xc.enc_y(1, 1), point(1037))   # x = 0 with the sign bit set: copied through as it came
    b = Block(a, signed=signed)
    b.add(range(0, 12))
    b.add(range(4, 16))
    b.add([15, 0, 14, 1, 13, 2, 12, 3, 11, 4, 10, 5])

    def also(block, verdicts, accounts, stats):
        assert accounts[16] == as_given(a[16]) and decode(a[16]["balance"][0])[0] == 0
        assert accounts[5]["flags"] == DUE | ROLLED and accounts[5]["balance"] == tuple(a[5]["balance"])   # + Ciphertext::zero()
    b.expect = dict(verdicts=["accepted"] * 3, rounds=1, proofs_verified=3, also=also)
    return b


def _key_twice_in_a_ring():
    a = [account(k, DUE if k in (2, 7) else 0) for k in range(11)]
    b = Block(a)
    ring = list(range(11)) + [2]   # members 2 and 11 are account 2, which is due
    b.add(ring)

    def also(block, verdicts, accounts, stats):
        x = block.xts[0]
        assert accounts[2]["flags"] == DUE | ROLLED
        assert accounts[2]["balance"] == sum_ct([a[2]["balance"], a[2]["pending"]])   # one rollover
        assert accounts[2]["pending"] == sum_ct([(x["left_ciphertexts"][2], x["right_ciphertext"]), (x["left_ciphertexts"][11], x["right_ciphertext"])])
        met = block.live.balances_met(x)   # (the model is past its rollover: these are the rolled balances)
        assert met[2] == met[11]
    b.expect = dict(verdicts=["accepted"], rounds=1, proofs_verified=1, also=also)
    return b


def _due_account_in_every_ring():
    a = [account(k, DUE if k in (0, 20) else 0) for k in range(24)]
    b = Block(a)
    b.add([0] + list(range(1, 12)))
    b.add(list(range(12, 17)) + [0] + list(range(17, 23)), proof="bad")
    b.add(list(range(6, 17)) + [0])

    def also(block, verdicts, accounts, stats):
        assert accounts[0]["flags"] == DUE | ROLLED and accounts[0]["balance"] == sum_ct([a[0]["balance"], a[0]["pending"]])
        x0, x2 = block.xts[0], block.xts[2]
        assert accounts[0]["pending"] == sum_ct([(x0["left_ciphertexts"][0], x0["right_ciphertext"]), (x2["left_ciphertexts"][11], x2["right_ciphertext"])])
        assert accounts[23] == as_given(a[23])
    b.expect = dict(verdicts=["accepted", "invalid proof", "accepted"], rounds=1, proofs_verified=3, also=also)
    return b


def _balances_do_not_move():
    a = [account(k, DUE if k % 4 == 1 else 0) for k in range(14)]
    b = Block(a)
    b.add(range(0, 12))
    b.add(range(2, 14))   # ten members of the first, which was accepted: their balances are what they were
    b.add(range(0, 12))
    b.expect = dict(verdicts=["accepted"] * 3, rounds=1, proofs_verified=3)
    return b


def _rejected(how):
    """an extrinsic rejected at the proof leaves its ring's due accounts rolled with zero pending; one rejected at the signature
    leaves its ring as it came"""
    a = [account(k, DUE if k < 12 and k % 3 == 0 else 0) for k in range(24)]
    b = Block(a)
    if how == "proof":
        b.add(range(0, 12), proof="bad")
    else:
        b.add(range(0, 12), sig="bad R" if how == "signature R" else "bad")
    b.add(range(12, 24))

    def also(block, verdicts, accounts, stats):
        for k in range(12):
            if how != "proof":
                assert accounts[k] == as_given(a[k]), k
            elif a[k]["flags"] & DUE:
                assert accounts[k]["flags"] == DUE | ROLLED and accounts[k]["pending"] == ZERO_CT
                assert accounts[k]["balance"] == sum_ct([a[k]["balance"], a[k]["pending"]])
            else:
                assert accounts[k] == as_given(a[k]), k
    b.expect = dict(verdicts=["invalid proof" if how == "proof" else "bad signature", "accepted"], rounds=1, proofs_verified=2 if how == "proof" else 1, also=also)
    return b


def _same_nonce(first_accepted):
    a = [account(k) for k in range(16)]
    b = Block(a, pool=[point(2900)])
    n = point(2901)
    b.add(range(0, 12), nonce=n, proof="valid" if first_accepted else "bad")
    b.add(range(4, 16), nonce=n)
    b.add(range(2, 14), nonce=point(2900))                              # a nonce the pool came with
    b.add(range(1, 13), nonce=point(2900), right_ciphertext=UNDECODABLE)   # ... together with a refused point: step 4 comes first
    b.add(range(3, 15))
    # the twin of an accepted nonce was in the batch: its proof was checked, and the sweep rejects it all the same
    b.expect = dict(verdicts=["accepted", "nonce used", "nonce used", "nonce used", "accepted"] if first_accepted else
                    ["invalid proof", "accepted", "nonce used", "nonce used", "accepted"], rounds=1, proofs_verified=3)
    return b


def _refused_fields(bad):
    """enc_keys[3] (an account under the bad key), left_ciphertexts[0], [5], [11], field 49, field 52, two in one extrinsic"""
    a = [account(k, DUE if k % 5 == 0 else 0) for k in range(13)]
    a.append(dict(enc_key=bad, balance=a[0]["balance"], pending=None, flags=0))
    b = Block(a)
    ring = list(range(12))
    b.add(ring[:3] + [13] + ring[4:])                       # field 4: enc_keys[3]
    b.add(ring, lefts={0: bad})                             # 13
    b.add(ring, lefts={5: bad})                             # 18
    b.add(ring, lefts={11: bad})                            # 24
    b.add(ring, right_ciphertext=bad)                       # 49
    b.add(ring, nonce=bad)                                  # 52
    b.add(range(1, 13))
    b.add(ring, right_ciphertext=bad, lefts={7: bad, 9: bad})   # three refused: the first in push order, 13 + 7
    st = decode(bad)[0]
    assert st in (2, 3)
    why = zk.INTO_XY_REASONS[st]
    ref = lambda k: ("refused point", (FIELDS[k - 1], why))
    assert FIELDS[3] == "enc_keys[3]" and FIELDS[12] == "left_ciphertexts[0]" and FIELDS[48] == "right_ciphertext" and FIELDS[51] == "nonce"
    b.expect = dict(verdicts=[ref(4), ref(13), ref(18), ref(24), ref(49), ref(52), ("accepted", None), ref(20)], rounds=1, proofs_verified=1)
    return b


def _refused_rvk_and_epoch(bad):
    a = [account(k) for k in range(14)]
    b = Block(a, signed=False, pool=[point(2900)])
    b.add(range(0, 12), rvk=bad)                                 # field 50 (unsigned: with signatures a bad rvk is a bad signature)
    e = Block(a, signed=False, pool=[point(2900)], g_epoch=bad)
    e.add(range(0, 12))                                          # field 51
    e.add(range(1, 13), lefts={11: bad})                         # field 24 comes first
    e.add(range(2, 14), nonce=point(2900))                       # a nonce in the pool wins over a refused g_epoch
    e.add(range(0, 12), nonce=bad)                               # field 51 before 52
    why = zk.INTO_XY_REASONS[decode(bad)[0]]
    b.expect = dict(verdicts=[("refused point", ("rvk", why))], rounds=1, proofs_verified=0)
    e.expect = dict(verdicts=[("refused point", ("g_epoch", why)), ("refused point", ("left_ciphertexts[11]", why)), ("nonce used", None),
                              ("refused point", ("g_epoch", why))], rounds=1, proofs_verified=0)
    return b, e


def _bad_accounts():
    a = [account(k, DUE if k in (0, 1, 12, 20, 25) else 0) for k in range(27)]
    a[4]["balance"] = (UNDECODABLE, a[4]["balance"][1])      # member 4 of extrinsic 0: its balance's left
    a[21]["pending"] = (a[21]["pending"][0], torsion())      # member 9 of extrinsic 1: its pending's right
    a[26]["pending"] = (torsion(), a[26]["pending"][1])      # named by nobody: copied through
    b = Block(a)
    b.add(range(0, 12))                      # account 0 is due and no other extrinsic names it: not rolled; 1 is due, and extrinsic 2 names it
    b.add(range(12, 24))                     # 12 and 20 are due; 12 is in extrinsic 2 as well
    b.add([1, 12, 24, 25] + list(range(5, 12)) + [13])

    def also(block, verdicts, accounts, stats):
        assert accounts[0] == as_given(a[0]) and accounts[20] == as_given(a[20])          # due, named by a BAD_ACCOUNT extrinsic only
        for k in (1, 12, 25):
            assert accounts[k]["flags"] == DUE | ROLLED, k
        for k in (4, 21):
            assert accounts[k]["balance"] == accounts[k]["pending"] == (bytes(32), bytes(32)) and accounts[k]["flags"] == a[k]["flags"]
        assert accounts[26] == as_given(a[26])
    b.expect = dict(verdicts=["bad account", "bad account", "accepted"], rounds=1, proofs_verified=1, also=also)
    return b


@functools.lru_cache(maxsize=None)
def cases():
    und = _refused_rvk_and_epoch(UNDECODABLE)
    tor = _refused_rvk_and_epoch(torsion())
    return {
        "honest": _honest(),
        "honest_unsigned": _honest(signed=False),
        "key_twice_in_a_ring": _key_twice_in_a_ring(),
        "due_account_in_every_ring": _due_account_in_every_ring(),
        "balances_do_not_move": _balances_do_not_move(),
        "rejected_at_the_proof": _rejected("proof"),
        "rejected_at_the_signature": _rejected("signature"),
        "rejected_at_the_signature_R": _rejected("signature R"),
        "same_nonce_first_accepted": _same_nonce(True),
        "same_nonce_first_invalid": _same_nonce(False),
        "refused_fields_undecodable": _refused_fields(UNDECODABLE),
        "refused_fields_torsion": _refused_fields(torsion()),
        "refused_rvk_undecodable": und[0],
        "refused_g_epoch_undecodable": und[1],
        "refused_rvk_torsion": tor[0],
        "refused_g_epoch_torsion": tor[1],
        "unreadable_accounts": _bad_accounts(),
    }


CASE_NAMES = ("honest", "honest_unsigned", "key_twice_in_a_ring", "due_account_in_every_ring", "balances_do_not_move", "rejected_at_the_proof",
              "rejected_at_the_signature", "rejected_at_the_signature_R", "same_nonce_first_accepted", "same_nonce_first_invalid",
              "refused_fields_undecodable", "refused_fields_torsion", "refused_rvk_undecodable", "refused_g_epoch_undecodable", "refused_rvk_torsion",
              "refused_g_epoch_torsion", "unreadable_accounts")


# ---------------------------------------------------------------------------------------------- running
def execute(lib, block):
    pvk = zk.prepare_verifying_key(small_anon_key()[1], lib=lib)
    try:
        return zk.execute_anonymous_block(pvk, *block.args())
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
    assert stats["rounds"] <= 1
    ex = block.expect
    if "verdicts" in ex:   # what the case was built to show, stated without the model
        assert [v if isinstance(w, tuple) else v[0] for v, w in zip(verdicts, ex["verdicts"])] == list(ex["verdicts"])
    for k in ("rounds", "proofs_verified"):
        if k in ex:
            assert stats[k] == ex[k], (k, stats)
    if "also" in ex:
        ex["also"](block, verdicts, accounts, stats)


def run_case(lib, name):
    block = cases()[name]
    check(block, execute(lib, block))


def _raw(lib, pvk, block, n=None, null=(), decreasing=False):
    """the entry through the ctypes handle, every output pre-filled with 0xAA: (status, accounts bytes, verdict bytes, stats bytes)"""
    xts, accounts, pool, ge, sigs, msgs = block.args()
    n = len(xts) if n is None else n
    arr = (zl.AnonymousXt * max(len(xts), 1))()
    for dst, x in zip(arr, xts):
        for f in ("proof", "right_ciphertext", "nonce", "rsk", "rvk"):
            getattr(dst, f)[:] = x[f]
        for f in ("enc_keys", "left_ciphertexts"):
            for k in range(RING):
                getattr(dst, f)[k][:] = x[f][k]
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
    if decreasing:
        offs[2] = offs[1] - 1
    ptr =lambda a: a.ctypes.data_as(C.c_void_p)
    arg = dict(xts=arr, sigs=None if sb is None else ptr(sb), msgs=None if mb is None else ptr(mb), offs=ptr(offs), accounts=acc, pool=ptr(pb) if pool else None,
               g_epoch=ptr(gb), out=C.cast(ptr(out), C.POINTER(zl.BlockAccount)), verdicts=C.cast(ptr(ver), C.POINTER(zl.BlockVerdict)),
               stats=C.cast(ptr(st), C.POINTER(zl.BlockStats)))
    for k in null:
        arg[k] = None
    status = lib.zk_anonymous_block_execute(pvk._h, n, arg["xts"], arg["sigs"], arg["msgs"], arg["offs"], len(accounts), arg["accounts"], len(pool), arg["pool"],
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
    pvk = zk.prepare_verifying_key(small_anon_key()[1], lib=lib)
    try:
        honest = cases()["honest"]
        untouched = lambda r: all(set(b) <= {0xAA} for b in r[1:])
        # a ring key that is not among the accounts (account 15 is member 11 of extrinsic 1 and member 0 of extrinsic 2)
        short = _OtherAccounts(honest, honest.accounts[:15] + honest.accounts[16:])
        r = _raw(lib, pvk, short)
        assert r[0] == 16 and untouched(r) and b"extrinsic 1" in lib.zk_last_error() and b"key 11" in lib.zk_last_error()
        # two accounts with equal keys
        twice = _OtherAccounts(honest, honest.accounts + [dict(honest.accounts[2], balance=None)])
        r = _raw(lib, pvk, twice)
        assert r[0] == 16 and untouched(r) and b"account 17" in lib.zk_last_error()
        # NULL buffers with non-zero counts
        for null in (("xts",), ("verdicts",), ("g_epoch",), ("accounts",), ("out",), ("pool",), ("offs",)):
            blk = cases()["same_nonce_first_accepted"] if null == ("pool",) else honest
            r = _raw(lib, pvk, blk, null=null)
            assert r[0] == 16 and untouched(r), null
        r = _raw(lib, pvk, honest, decreasing=True)
        assert r[0] == 16 and untouched(r) and b"msg_offsets decrease at 1" in lib.zk_last_error()
        assert _raw(lib, pvk, honest, null=("stats",))[0] == 0   # stats_out may be NULL
        # nothing to do: the accounts are copied through, flags and all, and no verdict is written
        r = _raw(lib, pvk, honest, n=0)
        acc = (zl.BlockAccount * len(honest.accounts)).from_buffer_copy(r[1])
        assert r[0] == 0 and set(r[2]) == {0xAA} and r[3] == bytes(16)
        for o, a in zip(acc, honest.accounts):
            assert bytes(o.enc_key) == a["enc_key"] and bytes(o.balance) == b"".join(a.get("balance") or ZERO_CT) and o.flags == a["flags"]
            assert bytes(o.pending) == b"".join(a.get("pending") or ZERO_CT)
        assert _raw(lib, pvk, honest, n=0, null=("xts", "verdicts", "g_epoch", "sigs", "msgs", "offs"))[0] == 0
        assert zk.execute_anonymous_block(pvk, [], [], [], honest.g_epoch) == ([], [], dict(rounds=0, proofs_verified=0, points_decoded=0))
    finally:
        pvk.close()
    # a key with 22 inputs
    pvk22 = zk.prepare_verifying_key(xc.small_conf_key()[1], lib=lib)
    try:
        assert pvk22.n_inputs == 22
        with pytest.raises(zk.ZkError) as e:
            zk.execute_anonymous_block(pvk22, *honest.args())
        assert e.value.variant == "MalformedVerifyingKey"
    finally:
        pvk22.close()


# ---------------------------------------------------------------------------------------------- the shapes of the device form
@functools.lru_cache(maxsize=None)
def rolled_accounts(r):
    """three extrinsics whose rings cover 36 accounts, the first r of them due: 2 r lanes of k_ring_balance_xy"""
    a = [account(40 + k, DUE if k < r else 0) for k in range(36)]
    b = Block(a, signed=False, first_point=8000)
    for i in range(3):
        b.add(range(12 * i, 12 * i + 12))

    def also(block, verdicts, accounts, stats):
        assert sum(bool(o["flags"] & ROLLED) for o in accounts) == r
    b.expect = dict(verdicts=["accepted"] * 3, rounds=1, proofs_verified=3, also=also)
    return b


@functools.lru_cache(maxsize=None)
def to_verify(nv):
    """nv extrinsics to verify and one that is not (its nonce is in the pool): 52 nv lanes of the rows' gather"""
    a = [account(40 + k, DUE if k % 2 else 0) for k in range(12 + nv)]
    b = Block(a, signed=False, pool=[point(2900)], first_point=8200)
    for i in range(nv):
        if i == 2:
            b.add(range(0, 12), nonce=point(2900))
        b.add(range(i, i + 12))
    b.expect = dict(verdicts=["accepted", "accepted", "nonce used"] + ["accepted"] * (nv - 2), rounds=1, proofs_verified=nv)
    return b


LARGE_N, LARGE_REJECTED = 30, 6


@functools.lru_cache(maxsize=None)
def large_block():
    """30 extrinsics over 40 accounts, six rejected for mixed reasons: 360 additions by index and the rollovers' ops, so the scan
    crosses a workgroup and slots straddle the boundary and take the carry"""
    a = [account(100 + k, DUE if k % 3 else 0) for k in range(40)]
    b = Block(a, pool=[point(2900)], first_point=8600)
    rejected = {3: dict(proof="bad"), 8: dict(sig="bad"), 13: dict(nonce=point(2900)), 17: dict(lefts={6: UNDECODABLE}), 22: dict(sig="bad R"),
                27: dict(right_ciphertext=torsion())}
    for i in range(LARGE_N):
        b.add([(7 * i + 3 * k) % 40 for k in range(RING)], **rejected.get(i, {}))
    got = [v[0] for v in b.live.verdicts]
    assert [i for i in range(LARGE_N) if got[i] != "accepted"] == sorted(rejected), got
    assert {got[i] for i in rejected} == {"invalid proof", "bad signature", "nonce used", "refused point"}
    b.expect = dict(rounds=1, proofs_verified=LARGE_N - 5)   # all but the two bad signatures, the pool's nonce and the two refusals
    return b
