"""What the batched-Merkle tests share (tests/test_merkle_batch_host.py on the CPU, tests/test_gpu_merkle_batch.py on the GPU): the shapes, the
inputs, the oracle's trees and its verify_many_ds / verify_pairs_ds over proof bytes (tests/oracle_merkle_verify.cpp, built here), and the tamperings."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (arity, n, pairs): every width (t = 17, 9, 9 as pairs, 65), one leaf, one node, a ragged last node, two levels with a ragged top
SHAPES = [(16, 1, False), (16, 2, False), (16, 16, False), (16, 17, False), (16, 257, False), (8, 65, False), (4, 64, True), (64, 65, False)]
BATCHES = [1, 3]


def leaves_of(oracle, seed, b, n):
    """column b of a batch: n elements in the stored form (the synthetic column generator of DESIGN "Synthetic inputs")"""
    return oracle.synth_column(seed, b, 0, n)


def labels_of(B, base=0x5EED):
    return [base + 7 * b for b in range(B)]


def index_lists(n, b):
    """index lists with duplicates and the last leaf (of a ragged node where the shape has one); list b differs from list b + 1"""
    ix = [n - 1, (3 * b) % n, n // 2, (3 * b) % n, 0 if b % 2 else n - 1]
    return ix


@functools.lru_cache(maxsize=None)
def oracle_tree(oracle, seed, b, arity, n, pairs, label, cp_zero):
    """the oracle's tree of column b (cached for the session and left unchanged); pairs: cp is column b + 100, or zeros"""
    f = leaves_of(oracle, seed, b, n)
    cp = None if not pairs else (np.zeros((n, 4), np.uint64) if cp_zero else leaves_of(oracle, seed, b + 100, n))
    return oracle.merkle_build(arity, label, f, cp)


@functools.lru_cache(maxsize=None)
def oracle_verify_lib():
    out = os.path.join(ROOT, "tests", "_build", "liboracle_merkle_verify.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fopenmp", "-fPIC", "-shared", "-Wno-unused-function", "-o", out, os.path.join(ROOT, "tests", "oracle_merkle_verify.cpp")])
    return C.CDLL(out)


def oracle_verify(cfg_arity, label, root, idx, values, proof: bytes, commitment=False):
    """the oracle's verify_many_ds over proof bytes: 1 accept, 0 reject, -1 where the reference would panic; commitment: under MerkleCommitment's
    parameters (arity 16, "POSEIDON-T17-X5-SEED": the trees of the sum-check proofs) instead of poseidon_params_for_arity(cfg_arity)"""
    ix = np.ascontiguousarray(idx, dtype=np.uint64); v = np.ascontiguousarray(values, dtype=np.uint64); r = np.ascontiguousarray(root, dtype=np.uint64)
    buf = (C.c_uint8 * max(1, len(proof))).from_buffer_copy(proof or b"\0")
    if commitment:
        assert cfg_arity == 16
        return oracle_verify_lib().om_verify_many_ds_commitment(C.c_uint64(label), r.ctypes.data_as(C.c_void_p), ix.ctypes.data_as(C.c_void_p), C.c_size_t(len(ix)),
                                                                v.ctypes.data_as(C.c_void_p), buf, C.c_size_t(len(proof)))
    return oracle_verify_lib().om_verify_many_ds(C.c_size_t(cfg_arity), C.c_uint64(label), r.ctypes.data_as(C.c_void_p), ix.ctypes.data_as(C.c_void_p), C.c_size_t(len(ix)),
                                                 v.ctypes.data_as(C.c_void_p), buf, C.c_size_t(len(proof)))


def oracle_verify_pairs(cfg_arity, label, root, idx, f, cp, proof: bytes):
    """the oracle's verify_pairs_ds over proof bytes: 1 accept, 0 reject, -1 where the reference would panic"""
    ix = np.ascontiguousarray(idx, dtype=np.uint64); r = np.ascontiguousarray(root, dtype=np.uint64)
    fv = np.ascontiguousarray(f, dtype=np.uint64).reshape(-1, 4); cv = np.ascontiguousarray(cp, dtype=np.uint64).reshape(-1, 4)
    buf = (C.c_uint8 * max(1, len(proof))).from_buffer_copy(proof or b"\0")
    return oracle_verify_lib().om_verify_pairs_ds(C.c_size_t(cfg_arity), C.c_uint64(label), r.ctypes.data_as(C.c_void_p), ix.ctypes.data_as(C.c_void_p), C.c_size_t(len(ix)),
                                                  fv.ctypes.data_as(C.c_void_p), cv.ctypes.data_as(C.c_void_p), buf, C.c_size_t(len(proof)))


def off8(a):
    """a copy of the uint64 array `a` whose first byte sits at an address that is 8 mod 16: what a caller's `&[F]` or a root held behind a u64
    in a struct may hand to the C-ABI (a uint64_t pointer promises no more than 8-byte alignment)"""
    a = np.ascontiguousarray(a, dtype=np.uint64); raw = np.zeros(a.size + 2, np.uint64)
    o = 1 if raw.ctypes.data % 16 == 0 else 0
    v = raw[o:o + a.size].reshape(a.shape); v[...] = a
    assert v.ctypes.data % 16 == 8
    return v


def flip_bit(a, word=0, bit=0):
    b = np.array(a, dtype=np.uint64, copy=True); b.reshape(-1)[word] ^= np.uint64(1 << bit); return b


def sibling_offset(idx):
    """byte offset of the first sibling element of a canonical MerkleProof that opens `idx` (or None: no sibling level 0)"""
    return 8 + 8 * len(set(int(i) for i in idx)) + 8 + 8


def tamperings(label, root, idx, values, proof: bytes, n):
    """(name, label, root, idx, values, proof) for the honest opening and each tampering of the issue's list"""
    idx = [int(i) for i in idx]
    out = [("honest", label, root, idx, values, proof),
           ("value bit", label, root, idx, flip_bit(values, 4 * (len(idx) - 1) + 1, 17), proof),
           ("wrong root", label, flip_bit(root, 2, 5), idx, values, proof),
           ("truncated", label, root, idx, values, proof[:-9]),
           ("empty", label, root, idx, values, b""),
           ("index out of range", label, root, idx[:-1] + [n + 3], values, proof)]
    so = sibling_offset(idx)
    if so + 32 <= len(proof) - 8 and int.from_bytes(proof[8 + 8 * len(set(idx)):so - 8], "little") > 0 and int.from_bytes(proof[so - 8:so], "little") > 0:
        b = bytearray(proof); b[so + 3] ^= 0x10
        out.append(("sibling bit", label, root, idx, values, bytes(b)))
    return out
