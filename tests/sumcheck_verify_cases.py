"""The mixed batches of the batched sum-check verifier tests (host and GPU): honest proofs of several shapes made by the oracle,
truncated / extended / empty ones, single-bit flips, an element forced out of the field, duplicates, and for verify_mf an honest
proof under a wrong label — each with the oracle's decision (channel/src/lib.rs:1080-1128, :1176-1240).  Not a test module."""
import random

PLAIN_SHAPES = [(6, 5050), (5, 2025), (1, 1)]                       # (k, label): tests/test_gpu_r2_sumcheck.py
MF_SHAPES = [(5, 6060, 3), (6, 11, 2), (3, 9, 8), (1, 4, 1)]        # (k, label, q)
FIXED_FLIPS = lambda n: [0, 7, 8, 39, 40, n - 1, n - 33]            # byte positions


def flips(p, seed, extra=50):
    rng = random.Random(seed)
    out = []
    for pos in FIXED_FLIPS(len(p)) + [rng.randrange(len(p)) for _ in range(extra)]:
        bad = bytearray(p); bad[pos] ^= 1 << rng.randrange(8); out.append(bytes(bad))
    return out


def out_of_field(p):
    """the first FBytes (8-byte length prefix, 32 bytes): its top byte forced to 0xFF, a value >= r"""
    bad = bytearray(p); bad[8 + 31] = 0xFF
    return bytes(bad)


_cache = {}


def mixed_batch(oracle, mf):
    """-> list of (proof bytes, k, label, q, honest) and the oracle's decisions"""
    if mf in _cache:
        return _cache[mf]
    items = []
    shapes = MF_SHAPES if mf else [(k, l, 0) for k, l in PLAIN_SHAPES]
    honest = []
    for i, (k, label, q) in enumerate(shapes):
        w = oracle.rand_fr_columns(40 + 3 * i + mf, 1 << k, 1)[0]
        honest.append((oracle.sumcheck_prove(mf, k, label, w, q=q or 2), k, label, q))
    for p, k, label, q in honest:
        items.append((p, k, label, q, True))
    p, k, label, q = honest[0]
    for bad in (b"", p[:-1], p + b"\0", p[:len(p) // 2]):
        items.append((bad, k, label, q, False))
    tampered = flips(p, 1000 + mf)
    for bad in tampered:
        items.append((bad, k, label, q, False))
    items.append((out_of_field(p), k, label, q, False))
    items.append((p, k, label, q, True)); items.append((tampered[3], k, label, q, False))      # duplicates
    if mf:
        items.append((p, k, label + 1, q, False))                                               # an honest proof under a wrong label
    else:
        items.append((p, honest[1][1], honest[1][2], q, True))                                  # another k and label: verify_plain reads neither
    want = [oracle.sumcheck_verify(mf, k, label, p, q=q or 2) == 1 for p, k, label, q, _ in items]
    _cache[mf] = (items, want)
    return _cache[mf]
