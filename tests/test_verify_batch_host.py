"""The batch verifier's plan (stark_mlwe_amd/csrc/fri_verify_batch.hpp: every hash of every opening of every proof recorded as a job over one
pool, grouped by Poseidon width and dependency depth) on the CPU: hc_deep_fri_verify_batch runs that plan through the host instantiation of
the kernel bodies the device runs (hash_ds_body over DsGatherStream, leaf_pair_body).  Each decision must equal the single call
(hc_deep_fri_verify: the same plan with one item) and, independently, the oracle's restatement of deep_fri_verify (fri.rs:643-762) on that proof alone.
The GPU build of the same plan (stark_deep_fri_verify_batch) is tested in tests/test_gpu_verify_batch.py."""
import ctypes as C
import random

import numpy as np
import pytest

SEED_Z = 0xDEEFBAAD
SHAPES = [(1 << 10, [16, 8], 8), (1 << 9, [8, 4, 2], 5), (1 << 11, [16, 16, 8], 6), (64, [8, 8], 4), (2, [2], 1)]


@pytest.fixture(scope="module")
def tparams(hostcheck):
    h = hostcheck.params(1)
    yield h
    hostcheck.params_free(h)


def verify_batch(hostcheck, tparams, proofs, sched, r):
    n = len(proofs)
    bufs = [(C.c_uint8 * max(1, len(p))).from_buffer_copy(p or b"\0") for p in proofs]
    ptrs = (C.c_void_p * max(1, n))(*[C.cast(b, C.c_void_p) for b in bufs])
    lens = (C.c_size_t * max(1, n))(*[len(p) for p in proofs])
    sch = np.ascontiguousarray(sched, dtype=np.uint64)
    acc = (C.c_int32 * max(1, n))()
    rc = hostcheck.l.hc_deep_fri_verify_batch(tparams, C.c_size_t(n), ptrs, lens, sch.ctypes.data_as(C.c_void_p), C.c_size_t(len(sched)), C.c_size_t(r), acc)
    assert rc == 0
    return [int(acc[i]) for i in range(n)]


def make_proof(oracle, n0, sched, r, seed):
    cols = oracle.rand_fr_columns(seed, n0, 4)
    ref = oracle.deep_fri_prove(cols[0], cols[1], cols[2], cols[3], n0, sched, r, SEED_Z)
    b = ref.bytes(); ref.free()
    return b


@pytest.mark.parametrize("n0,sched,r", SHAPES)
def test_batch_decisions_equal_single_and_oracle(oracle, hostcheck, tparams, n0, sched, r):
    proof = make_proof(oracle, n0, sched, r, 77 + n0)
    other_n0 = make_proof(oracle, 2 * n0, sched, r, 91 + n0)                  # another n0 under the same schedule: accepted on its own
    foreign = [make_proof(oracle, *s, 5) for s in SHAPES if s[1] != sched][:1]  # a proof of another schedule: rejected
    batch = [proof, other_n0, b"", proof[:-1], proof + b"\0", proof[: len(proof) // 2], other_n0[:-8]] + foreign
    rng = random.Random(n0 * 7 + r)
    positions = sorted(set([0, 7, 8, 8 + 31, 40, len(proof) - 1, len(proof) - 33, len(proof) - 41] + [rng.randrange(len(proof)) for _ in range(40)]))
    assert len(positions) >= 40
    for pos in positions:
        bad = bytearray(proof); bad[pos] ^= 1 << rng.randrange(8); batch.append(bytes(bad))
    batch += [proof, batch[8], batch[-1]]                                      # duplicates: the same bytes twice in one batch
    want = [1 if oracle.deep_fri_verify(p, sched, r, SEED_Z) == 1 else 0 for p in batch]
    single = [hostcheck.deep_fri_verify(tparams, p, sched, r) for p in batch]
    assert single == want
    assert want[0] == want[1] == 1 and want[2:7] == [0] * 5 and 0 < sum(want) < len(want) // 2
    got = verify_batch(hostcheck, tparams, batch, sched, r)
    assert got == want, [i for i in range(len(batch)) if got[i] != want[i]]
    assert verify_batch(hostcheck, tparams, batch[::-1], sched, r) == want[::-1]
    for p in (proof, other_n0, batch[8], b""):
        assert verify_batch(hostcheck, tparams, [p], sched, r) == [hostcheck.deep_fri_verify(tparams, p, sched, r)]
    assert verify_batch(hostcheck, tparams, [proof, other_n0], sched, r + 1) == [0, 0]      # wrong parameters reject every proof
    assert verify_batch(hostcheck, tparams, [proof, other_n0], sched[:-1], r) == [0, 0]


def test_batch_first_payload_wins_and_local_check(oracle, hostcheck, tparams):
    """Repeated query indices (fri.rs:663-664: the FIRST payload is hashed) and the local check s_i == f_parent_b (:168-176), in one batch:
    every fifth byte of the first three queries flipped once, decisions equal to the oracle's (the single call is this planner with one item: it is
    compared too, but it is no independent witness)."""
    n0, sched, r = 64, [8, 8], 24
    proof = make_proof(oracle, n0, sched, r, 5)
    per_q = 8 + 2 * 32 + 8 + len(sched) * 32 + 8 + len(sched) * 128
    qbase = len(proof) - 40 - r * per_q
    batch = [proof]
    for pos in range(qbase, qbase + 3 * per_q, 5):
        bad = bytearray(proof); bad[pos] ^= 4; batch.append(bytes(bad))
    want = [1 if oracle.deep_fri_verify(p, sched, r, SEED_Z) == 1 else 0 for p in batch]
    assert 1 < sum(want) < len(batch)
    assert verify_batch(hostcheck, tparams, batch, sched, r) == want
    assert [hostcheck.deep_fri_verify(tparams, p, sched, r) for p in batch] == want


def test_batch_empty(hostcheck, tparams):
    assert verify_batch(hostcheck, tparams, [], [16, 8], 8) == []
