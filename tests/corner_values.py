"""Input families for the stored-limb corner tests (test infrastructure, plain Python + numpy).

Field elements cross every boundary of this project as four u64 limbs in Montgomery form, and the delicate kernel arithmetic (lazy nine-limb
butterflies, fr29_partial_reduce, the wide dots' carry passes, the signed radix-256 recoding in front of the int8 matrix cores) is sensitive
to those STORED limbs.  A corner of the logical value passed through `from_int` reaches the code as ordinary random-looking words; the values
here are corners of the stored limbs themselves, and `sbox_preimage` / `crafted_children` / `crafted_state` place chosen stored words behind
the first S-box, where the recoding reads them."""
import math

import numpy as np

import pyref

R = pyref.R
M64 = (1 << 64) - 1
M29 = (1 << 29) - 1
SBOX_SHIFT = 20          # fr29.hpp FR29_SBOX_SHIFT: the kernels' S-box fr_pow5_r29 delivers the stored limbs of x^5 divided by 2^20


def raw(v):
    """integer -> four u64 limbs AS STORED (no Montgomery conversion)"""
    assert 0 <= v < 1 << 256
    return np.array([(v >> (64 * i)) & M64 for i in range(4)], np.uint64)


def raw_to_int(a):
    a = np.asarray(a, np.uint64).reshape(4)
    return sum(int(a[i]) << (64 * i) for i in range(4))


def raw_array(vals):
    """list of integers -> (n, 4) uint64 array of stored limbs"""
    return np.stack([raw(v) for v in vals]) if len(vals) else np.zeros((0, 4), np.uint64)


def hex_limbs(a):
    """stored limbs of one element or of an array of elements, as hex strings (for assertion messages)"""
    a = np.asarray(a, np.uint64).reshape(-1, 4)
    return ["%064x" % raw_to_int(x) for x in a]


def _from_bytes_le(bs):
    assert len(bs) == 32
    return int.from_bytes(bytes(bs), "little")


def carry_chains():
    """0x80 followed by 0x7f bytes up to byte 30 (top byte 0): adding 0x80 to every byte carries out of the first byte and through every later
    one — the longest carry chain of recode_signed, across all seven 32-bit word boundaries — and the same chain started at byte offsets 3, 4, 7."""
    return [_from_bytes_le([0] * off + [0x80] + [0x7f] * (30 - off) + [0]) for off in (0, 3, 4, 7)]


def alt29(phase):
    """maximal 29-bit limbs at the even (phase 0) or odd (phase 1) limb positions, zero between them, clipped to 254 bits"""
    return sum(M29 << (29 * i) for i in range(9) if i % 2 == phase) & ((1 << 254) - 1)


def alt32(phase):
    """0xffffffff at the even (phase 0) or odd (phase 1) 32-bit words, zero between them, clipped to 254 bits"""
    return sum(0xffffffff << (32 * i) for i in range(8) if i % 2 == phase) & ((1 << 254) - 1)


def stored_corners(p):
    """Stored values (integers below p, to be passed through `raw`), without duplicates, in a fixed order."""
    top = (p >> 248) - 1                                     # the largest top byte that keeps any lower bytes below p
    vals = [0, 1, 2, p - 1, p - 2, (1 << 254) - 1, 1 << 254, (1 << 254) + 1, R % p, p - R % p, (p - 1) // 2]
    vals += [_from_bytes_le([b] * 31 + [min(b, top)]) for b in (0x7f, 0x80, 0x81, 0xfe, 0xff, 0x01)]
    vals += carry_chains()
    vals += [alt29(0), alt29(1), alt32(0), alt32(1)]
    for k in (28, 29, 31, 32, 57, 58, 63, 64, 231, 232, 253):
        vals += [1 << k, (1 << k) - 1]
    out = []
    for v in vals:
        assert 0 <= v < p, hex(v)
        if v not in out:
            out.append(v)
    return out


def pattern_d(p, n):
    """i -> stored_corners(p)[i mod len] as an (n, 4) array"""
    c = raw_array(stored_corners(p))
    return c[np.arange(n) % c.shape[0]]


def patterns(p, n):
    """the named whole-vector patterns of the NTT / fold / sum-check tests: {name: (n, 4) stored array}"""
    i = np.arange(n)
    two = lambda a, b: raw_array([a, b])[i & 1]
    return {"all p-1": np.tile(raw(p - 1), (n, 1)), "all 2^254-1": np.tile(raw((1 << 254) - 1), (n, 1)),
            "alternating p-1 / 0": two(p - 1, 0), "alternating 29-bit limb phases": two(alt29(0), alt29(1)), "corners by index": pattern_d(p, n)}


# ---- chosen stored words behind the first S-box -----------------------------------------------------------------------------------
def stored_rc(params, r, i, p=pyref.P_PALLAS):
    """round constant i of full round r of a pyref parameter set (canonical integers), as the kernels hold it"""
    return params["rc_full"][r][i] * R % p


def sbox_preimage(stored_target, rc_stored, p=pyref.P_PALLAS, shift=SBOX_SHIFT):
    """the stored x for which the kernels' S-box fr_pow5_r29(x + rc) has exactly `stored_target` as its stored limbs — the limbs the signed
    radix-256 recoding reads.  fr_pow5_r29 takes three Montgomery steps by 2^261 on operands carrying R = 2^256, so it returns the stored limbs
    of x^5 divided by 2^20 (the matrices carry the 2^20); shift = 0 gives the preimage under a plain Montgomery x^5."""
    assert math.gcd(5, p - 1) == 1
    y = (stored_target << shift) * pow(R, -1, p) % p         # logical S-box output
    u = pow(y, pow(5, -1, p - 1), p)                         # logical S-box input
    return (u * R - rc_stored) % p


def crafted_state(params, targets, p=pyref.P_PALLAS):
    """a whole state (t stored integers) whose round-0 S-box outputs are the t given stored targets"""
    assert len(targets) == params["t"]
    return [sbox_preimage(tg, stored_rc(params, 0, i, p), p) for i, tg in enumerate(targets)]


def crafted_children(params, targets, p=pyref.P_PALLAS, tail=None):
    """The t - 1 children (stored integers) of a full node of hash_with_ds_dynamic such that in round 0 of the first permutation the S-box
    outputs of state elements 4..t-2 (children 0..t-6: elements 0..3 are the DS words, t-1 the capacity) are the given stored targets.  The last
    four children, absorbed after the first permutation, are `tail` (default: the first stored corners)."""
    t = params["t"]
    assert len(targets) == t - 5
    tail = stored_corners(p)[:4] if tail is None else list(tail)
    assert len(tail) == 4
    return [sbox_preimage(tg, stored_rc(params, 0, 4 + j, p), p) for j, tg in enumerate(targets)] + tail


def crafted_level(params, nodes, p=pyref.P_PALLAS, corners=None, last_children=None):
    """A Merkle level of `nodes` crafted nodes of arity t - 1: node n takes the corner list rotated by n — target of slot j = corners[(n + j) % L],
    tail children from the following positions — so that over any L consecutive nodes every corner meets every controllable slot.  `last_children`
    truncates the last node (a ragged level).  Returns ((n_children, 4) stored array, (nodes, t - 5) array of corner indices per slot)."""
    t = params["t"]; ns = t - 5
    corners = stored_corners(p) if corners is None else corners
    L = len(corners)
    pre = raw_array([sbox_preimage(c, stored_rc(params, 0, 4 + j, p), p) for j in range(ns) for c in corners]).reshape(ns, L, 4)
    cr = raw_array(corners)
    n = np.arange(nodes)[:, None]
    slot_idx = (n + np.arange(ns)[None, :]) % L
    tail_idx = (n + ns + np.arange(4)[None, :]) % L
    ch = np.concatenate([pre[np.arange(ns)[None, :], slot_idx], cr[tail_idx]], axis=1)        # (nodes, t - 1, 4)
    ch = np.ascontiguousarray(ch.reshape(-1, 4))
    if last_children is not None:
        ch = ch[:(nodes - 1) * (t - 1) + last_children].copy()
    return ch, slot_idx


def ds_words(oracle, arity, level, pos0, label, nodes):
    """the four DS words [arity, level, pos0 + k, label] of every node of a level, as an (nodes * 4, 4) array"""
    a, l, lb = oracle.from_u64(arity), oracle.from_u64(level), oracle.from_u64(label)
    return np.stack([x for k in range(nodes) for x in (a, l, oracle.from_u64(pos0 + k), lb)])


def mds_pre_canonical(params, p=pyref.P_PALLAS):
    """B_1 * M of the sparse partial-round factorisation (M_R = M, M_{k-1} = diag(1, Mhat_k) * M with Mhat_k = M_k[1:, 1:]), canonical integers"""
    t, M = params["t"], params["mds"]
    cur = [row[:] for row in M]
    for _ in range(params["rp"]):
        nxt = [M[0][:]]
        for i in range(1, t):
            nxt.append([sum(cur[i][q] * M[q][j] for q in range(1, t)) % p for j in range(t)])
        cur = nxt
    return cur
