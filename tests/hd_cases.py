"""A Python model of the hierarchical key derivation (zface/src/derive/mod.rs, components.rs; the account step
core/proofs/src/no_std_aliases/keys.rs:166-198) for tests/test_hd_derive.py: hashlib's BLAKE2 with person=, oracle/jubjub.py for the
points and oracle/gen_proof.py derive for the account of a spending key.

The reference holds no byte vectors for this module, so the model answers to it in three ways (tests/test_hd_derive.py): the
reference's own three invariants (derive/mod.rs:267-319) are asserted on the LIBRARY's outputs; the one pin the reference has for
gen_proof.derive - the encryption key of the seed "Alice" + 27 spaces - holds for the function the library's account step is compared
with, and is reached through the kernels' multiplier (a parent whose child has that seed's key cannot be built: f hashes the
parent's own key); and the byte pins below anchor regressions.  PINS were recorded from THIS model, not from the reference."""
import hashlib

from oracle import gen_proof as gp
from oracle import jubjub as jj

XSK, XPGK = 0, 1
HARDENED = 1 << 31
G = jj.note_commitment_randomness_generator()


def prf_expand_vec(sk, *parts):
    return hashlib.blake2b(bytes(sk) + b"".join(bytes(p) for p in parts), digest_size=64, person=b"zech_ExpandSeed_").digest()


def to_uniform(b):
    return int.from_bytes(b, "little") % jj.FS_MOD


def unpack(xkey):
    """(depth, tag, index, chain code, key bytes)"""
    assert len(xkey) == 73
    return xkey[0], xkey[1:5], int.from_bytes(xkey[5:9], "little"), xkey[9:41], xkey[41:73]


def pack(depth, tag, index, chain, key):
    return bytes([depth]) + bytes(tag) + index.to_bytes(4, "little") + bytes(chain) + bytes(key)


def master(seed):
    i = hashlib.blake2b(bytes(seed), digest_size=64, person=b"Zerochain_Master").digest()
    return pack(0, bytes(4), 0, i[32:], gp.spending_key_from_seed(i[:32]).to_bytes(32, "little"))


def xpgk_of(xsk):
    depth, tag, index, chain, key = unpack(xsk)
    return pack(depth, tag, index, chain, jj.write_point(jj.mul(G, int.from_bytes(key, "little"))))


def tag_of(pgk_bytes):
    return hashlib.blake2b(pgk_bytes, digest_size=32, person=b"ZerochainEFinger").digest()[:4]


def f_and_chain(chain, sk_bytes, pgk_bytes, index):
    i_le = index.to_bytes(4, "little")
    i = prf_expand_vec(chain, b"\x11", sk_bytes, i_le) if index >= HARDENED else prf_expand_vec(chain, b"\x12", pgk_bytes, i_le)
    return to_uniform(prf_expand_vec(i[:32], b"\x13")), i[32:]


def account_of(pgk_bytes):
    """(dec_key, enc_key bytes) of the 32 bytes of a proof generation key"""
    d = bytearray(hashlib.blake2s(pgk_bytes, digest_size=32, person=b"zech_bdk").digest())
    d[31] &= 0b00000111
    dk = int.from_bytes(d, "little")
    return dk, jj.write_point(jj.mul(G, dk))


def derive(kind, xkey, indices):
    """(xkeys, dec_keys, enc_keys) of the children `indices`, each child by the formula of ITS route: sk + f and the account of
    that spending key on the xsk route (gen_proof.derive), [f]G + pgk on the xpgk route"""
    depth, _, _, chain, key = unpack(xkey)
    assert depth < 255
    if kind == XSK:
        sk = int.from_bytes(key, "little")
        assert sk < jj.FS_MOD
        pgk_bytes = jj.write_point(jj.mul(G, sk))
    else:
        assert all(i < HARDENED for i in indices)
        pgk = jj.read_point(key)
        assert pgk is not None
        pgk_bytes = jj.write_point(pgk)
    tag = tag_of(pgk_bytes)
    memo, xkeys, dks, encs = {}, [], [], []
    for index in indices:
        if index not in memo:
            f, child_chain = f_and_chain(chain, key, pgk_bytes, index)
            if kind == XSK:
                child_sk = (sk + f) % jj.FS_MOD
                _, dk, enc = gp.derive(child_sk)
                memo[index] = (pack(depth + 1, tag, index, child_chain, child_sk.to_bytes(32, "little")), dk, jj.write_point(enc))
            else:
                child = jj.write_point(jj.add(jj.mul(G, f), pgk))
                memo[index] = (pack(depth + 1, tag, index, child_chain, child),) + account_of(child)
        x, dk, enc = memo[index]
        xkeys.append(x)
        dks.append(dk)
        encs.append(enc)
    return xkeys, dks, encs


# ---- regression anchors, recorded from the model above (NOT from the reference) for the seed bytes(range(32)): the master xsk,
# its children 0 and 2^31 + 3 on the xsk route, and their accounts
PIN_SEED = bytes(range(32))
PIN_MASTER = bytes.fromhex("0000000000000000004299737a62fa110910623e25bbb84543a2de0d947c3f177b6b1f2562e3a7a7397907e32232c2abe35b4c872a0b728b3d"
                           "4532262ca0da34a3b08be7bfe49c850a")
PIN_INDICES = [0, HARDENED + 3]
PIN_CHILDREN = [
    bytes.fromhex("0112463f2c0000000014244ca6046c0bb71191c58582dafd956f2065790808a9cce712d89af781e8611b5d45e7bb28e7a7aa5e0440cdbae9d6fab5"
                  "15ed065d7c0294760f05765f9a0d"),
    bytes.fromhex("0112463f2c03000080b4008dc3f6bbd648a2569989ab06c4b6d9ad1e591d5c8d5f2d3c8ef680f20389b853040bf072d199804c57e0219a58c3f6"
                  "362b4056b5901d7738d5ecf85c870b")]
PIN_DEC_KEYS = [0x6d3e3ef40cfa614a8ede8be9ad8a888e6cdc9dec489043531a9ffb273475172, 0x107e444bfa8086da9d854c90db6b271a2f9f0375b13a37f03240f0e971d4606]
PIN_ENC_KEYS = [bytes.fromhex("f8c33b53c9058f8c7becc74badc5a68beba9c6b96edf99bc7ddfe57aedd9e0e1"),
                bytes.fromhex("8980e44ef68aaa2d8647ddb48a7680445485d79553261360453c9a857643dd72")]


def booth_digits(k, width=6, windows=43):
    """the signed digits the kernels' fixed_mul walks (csrc/redjubjub.h booth_digit): digit w is
    -2^(width-1) b[pos + width - 1] + sum_j 2^j b[pos + j] + b[pos - 1] at pos = width * w; they sum to k below 2^252"""
    bit = lambda i: (k >> i) & 1 if i >= 0 else 0
    out = []
    for w in range(windows):
        pos = width * w
        out.append(sum(bit(pos + j) << j for j in range(width - 1)) + bit(pos - 1) - (bit(pos + width - 1) << (width - 1)))
    assert sum(d << (width * w) for w, d in enumerate(out)) == k
    return out
