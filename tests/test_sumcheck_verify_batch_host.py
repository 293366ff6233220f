"""The batched sum-check verifiers (stark_mlwe_amd/csrc/sumcheck_verify_batch.hpp) on the CPU: the planner over proof bytes and the plan's
device steps run through the host instantiation of the bodies the kernels run (sc_decode_fr, tr_batch_body over TrBatchStream, hash_ds_body
over DsGatherStream with MerkleCommitment's parameters, sc_check_plain / sc_check_mf).  Every decision must equal the oracle's verify_plain
/ verify_mf on that proof alone.  The GPU build of the same plan is tested in tests/test_gpu_sumcheck_verify_batch.py."""
import ctypes as C
import random

import numpy as np
import pytest

import pyref
import sumcheck_verify_cases as cases

vp = C.c_void_p


@pytest.fixture(scope="module")
def tparams(hostcheck):
    h = hostcheck.params(1)
    yield h
    hostcheck.params_free(h)


@pytest.fixture(scope="module")
def cparams(hostcheck):
    h = hostcheck.params(2, 17, b"POSEIDON-T17-X5-SEED")
    yield h
    hostcheck.params_free(h)


def _args(proofs, labels):
    n = len(proofs)
    bufs = [(C.c_uint8 * max(1, len(p))).from_buffer_copy(p or b"\0") for p in proofs]
    ptrs = (vp * max(n, 1))(*[C.cast(b, vp) for b in bufs])
    lens = (C.c_size_t * max(n, 1))(*[len(p) for p in proofs])
    lab = None if labels is None else np.ascontiguousarray(list(labels) or [0], dtype=np.uint64)
    return bufs, ptrs, lens, lab


def verify_batch(hostcheck, tparams, cparams, mf, proofs, labels):
    n = len(proofs)
    bufs, ptrs, lens, lab = _args(proofs, labels)
    acc = (C.c_int32 * max(n, 1))(*([7] * max(n, 1)))
    assert hostcheck.l.hc_sumcheck_verify_batch(tparams, cparams, mf, C.c_size_t(n), ptrs, lens, None if lab is None else lab.ctypes.data_as(vp), acc) == 0
    return [acc[i] == 1 for i in range(n)]


def plan_steps(hostcheck, mf, proofs, labels):
    n = len(proofs); cap = 256
    bufs, ptrs, lens, lab = _args(proofs, labels)
    kind, count = (C.c_int32 * cap)(), (C.c_size_t * cap)()
    hostcheck.l.hc_sumcheck_verify_batch_steps.restype = C.c_size_t
    g = hostcheck.l.hc_sumcheck_verify_batch_steps(mf, C.c_size_t(n), ptrs, lens, None if lab is None else lab.ctypes.data_as(vp), kind, count, C.c_size_t(cap))
    assert 0 < g <= cap
    return [(kind[i], count[i]) for i in range(g)]


@pytest.mark.parametrize("mf", [0, 1])
def test_mixed_batch_equals_oracle(hostcheck, tparams, cparams, oracle, mf):
    items, want = cases.mixed_batch(oracle, mf)
    proofs = [it[0] for it in items]; labels = [it[2] for it in items]
    # non-vacuity: every honest proof is accepted, and acceptances are a minority
    assert all(w for it, w in zip(items, want) if it[4])
    assert 0 < sum(want) < len(want) // 2
    assert sum(1 for it in items if it[0] != items[0][0] and len(it[0]) == len(items[0][0])) >= 50      # the single-bit flips
    got = verify_batch(hostcheck, tparams, cparams, mf, proofs, labels if mf else None)
    assert got == want, [i for i in range(len(want)) if got[i] != want[i]]
    assert verify_batch(hostcheck, tparams, cparams, mf, proofs[::-1], labels[::-1] if mf else None) == want[::-1]
    for i in (0, 1, len(cases.MF_SHAPES if mf else cases.PLAIN_SHAPES), 10, len(items) - 1):
        assert verify_batch(hostcheck, tparams, cparams, mf, [proofs[i]], [labels[i]]) == [want[i]], i
    assert verify_batch(hostcheck, tparams, cparams, mf, [], []) == []


def test_oracle_facts_on_labels(hostcheck, tparams, cparams, oracle):
    """verify_plain reads neither k nor the label; verify_mf hashes every opening under the label"""
    items, want = cases.mixed_batch(oracle, 0)
    p, k, label = items[0][0], items[0][1], items[0][2]
    assert oracle.sumcheck_verify(0, k + 3, label + 17, p) == 1 and items[-1][0] == p and want[-1] is True
    assert verify_batch(hostcheck, tparams, cparams, 0, [p, p], None) == [True, True]           # the plain call takes no labels
    items, want = cases.mixed_batch(oracle, 1)
    p, k, label, q = items[0][:4]
    assert oracle.sumcheck_verify(1, k, label + 1, p, q=q) == 0 and items[-1][0] == p and want[-1] is False
    assert verify_batch(hostcheck, tparams, cparams, 1, [p, p], [label, label + 1]) == [True, False]


@pytest.mark.parametrize("mf", [0, 1])
def test_step_count_does_not_depend_on_the_batch(hostcheck, oracle, mf):
    items, _ = cases.mixed_batch(oracle, mf)
    p, label = items[0][0], items[0][2]
    one = plan_steps(hostcheck, mf, [p], [label]); many = plan_steps(hostcheck, mf, [p] * 32, [label] * 32)
    assert len(one) == len(many)
    assert [k for k, _ in one] == [k for k, _ in many]
    assert all(c32 == 32 * c1 for (_, c1), (_, c32) in zip(one, many))
    assert {0, 1, 3} <= {k for k, _ in one} and (not mf or 2 in {k for k, _ in one})


def test_decode_body(hostcheck):
    """sc_decode_fr against from_le_bytes_mod_order: 0, 1, r - 1; r and 2^256 - 1 rejected; random values at every byte alignment"""
    r = pyref.P_PALLAS
    f = hostcheck.l.hc_sc_decode_fr

    def decode(blob, off):
        out = np.zeros(4, np.uint64); buf = (C.c_uint8 * len(blob)).from_buffer_copy(blob)
        return f(buf, C.c_size_t(len(blob)), C.c_size_t(off), out.ctypes.data_as(vp)), out

    for x in (0, 1, r - 1):
        rc, out = decode(x.to_bytes(32, "little"), 0)
        assert rc == 1 and (out == hostcheck.from_le_bytes_mod_order(x.to_bytes(32, "little"))).all(), x
    for x in (r, r + 1, 2**256 - 1, 0xFF << 248):
        assert decode(x.to_bytes(32, "little"), 0)[0] == 0, x
    rng = random.Random(11)
    for off in range(8):
        for _ in range(8):
            x = rng.randrange(r); noise = bytes(rng.randrange(256) for _ in range(off)) ; tail = bytes(rng.randrange(256) for _ in range(rng.randrange(0, 9)))
            rc, out = decode(noise + x.to_bytes(32, "little") + tail, off)
            assert rc == 1 and (out == hostcheck.from_le_bytes_mod_order(x.to_bytes(32, "little"))).all(), (off, x)
        x = rng.randrange(r, 2**256); noise = bytes(rng.randrange(256) for _ in range(off))
        assert decode(noise + x.to_bytes(32, "little"), off)[0] == 0
    assert decode(bytes(40), 9)[0] == -1                                                         # the element must lie inside the blob
