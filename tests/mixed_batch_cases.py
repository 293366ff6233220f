"""What the mixed-size batch tests share (tests/test_mixed_batch_host.py on the CPU, tests/test_gpu_mixed_batch.py on the GPU): the shape sets of
stark_merkle_build_mixed_batch_dev, the inputs and the oracle's trees (through merkle_batch_cases.oracle_tree, cached and left unchanged), and the round
counts and witnesses of the mixed-size sum-check proves.  No tests."""
import merkle_batch_cases as mc

SEED = 0x313D
# arity -> the n of one batch call.  Arity 16: one level only (n = 1, twice), a ragged last node at every depth (17 and 37 at level 1; 257 and 300
# at level 1, 17 and 19 at level 2; 4097 -> 257 -> 17 -> 2 -> 1), trees that leave at different levels, and levels whose only ragged node has a single
# child (17 -> 2 nodes, 257 -> 17 nodes -> 2 nodes, 4097 -> 257).  Arity 8 is the t = 9 form, arity 32 the wide form (t = 33).
SETS = {16: [1, 2, 16, 17, 37, 256, 257, 300, 1, 4097], 8: [1, 8, 9, 65, 513], 32: [1, 33, 1025]}
# one arity-16 call whose first node level has more than 4096 hashes (the wave pair), the next at most 4096 (one wave per node) and the rest at most
# 256 (five waves per node): 4375 + 257 + 2 + 1 + 19, then 274 + 17 + 2, then 18 + 2, then 2 + 1, then 1
THRESHOLDS = [70000, 4097, 17, 1, 300]


def labels_of(B):
    return mc.labels_of(B, base=0x31D)


def cp_is_null(b):
    """the pair batches: every third tree has a NULL cp entry (a zero column)"""
    return b % 3 == 1


def leaves_of(oracle, b, n):
    return mc.leaves_of(oracle, SEED, b, n)


def cps_of(oracle, ns):
    return [None if cp_is_null(b) else mc.leaves_of(oracle, SEED, b + 100, n) for b, n in enumerate(ns)]


def oracle_tree(oracle, arity, b, n, pairs, label):
    return mc.oracle_tree(oracle, SEED, b, arity, n, pairs, label, bool(pairs and cp_is_null(b)))


# sum-check: the round counts of one mixed call (two witnesses without a round, equal counts apart from each other, the largest not first) and the
# same witnesses in another order
SUMCHECK_K = [0, 1, 5, 3, 5, 0, 2]
SUMCHECK_SHUFFLE = [4, 6, 0, 3, 5, 2, 1]                                    # position -> index into SUMCHECK_K
SUMCHECK_LABELS = [2025, 7, 2025, 11, 6060, 5, 7]


def witnesses_of(oracle, ks, seed=0x5C):
    """witness i of a mixed call: 2^ks[i] elements (stored form), distinct per index"""
    return [oracle.rand_fr_columns(seed + 31 * i + k, 1 << k, 1)[0] for i, k in enumerate(ks)]
