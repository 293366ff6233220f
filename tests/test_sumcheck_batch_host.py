"""The batched sum-check provers (stark_mlwe_amd/csrc/sumcheck_batch.hpp) on the CPU: the round loops of prove_plain / prove_mf over B witnesses,
run through the host instantiation of the kernel bodies the device runs (hash_ds_body over DsBatchStream, tr_batch_body over TrBatchStream).
Every proof must equal the oracle's restatement of crates/channel/src/lib.rs on that witness alone.  The two new streams are also checked on
their own: one Merkle level of B trees against hc_hash_ds_level tree by tree, and B transcripts with ragged segments, pool gathers and a subset
launch against the pure-Python transcript.  The GPU build of the same drivers is tested in tests/test_gpu_sumcheck_batch.py."""
import ctypes as C
import random

import numpy as np
import pytest

import pyref

vp = C.c_void_p


def ptr(a):
    return a.ctypes.data_as(vp)


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


def prove_batch(hostcheck, tparams, cparams, mf, k, labels, witnesses, q=0):
    B = len(witnesses)
    ws = [np.ascontiguousarray(w, dtype=np.uint64) for w in witnesses]
    wp = (vp * B)(*[ptr(w) for w in ws])
    lab = np.ascontiguousarray(labels, dtype=np.uint64)
    lens = (C.c_size_t * B)()
    f = hostcheck.l.hc_sumcheck_prove_batch
    f.restype = C.c_size_t
    args = (tparams, cparams, mf, C.c_size_t(B), wp, C.c_size_t(k), ptr(lab), C.c_size_t(q))
    tot = f(*args, None, C.c_size_t(0), lens)
    assert tot > 0
    buf = (C.c_uint8 * tot)()
    assert f(*args, buf, C.c_size_t(tot), lens) == tot
    out, o = [], 0
    for b in range(B):
        out.append(bytes(buf[o:o + lens[b]])); o += lens[b]
    return out


@pytest.mark.parametrize("k", [0, 1, 3, 5])
def test_plain_batch_equals_oracle(hostcheck, tparams, cparams, oracle, k):
    labels = [2025, 7, 2025]
    ws = oracle.rand_fr_columns(100 + k, 1 << k, 3)
    got = prove_batch(hostcheck, tparams, cparams, 0, k, labels, ws)
    for b in range(3):
        assert got[b] == oracle.sumcheck_prove(0, k, labels[b], ws[b]), b
    if k > 0:
        assert len(set(got)) == 3


@pytest.mark.parametrize("k,q", [(0, 2), (1, 1), (3, 2), (3, 8), (5, 3), (2, 4)])
def test_mf_batch_equals_oracle(hostcheck, tparams, cparams, oracle, k, q):
    """(3, 8) and (2, 4): q >= half, so the duplicate redraws and the fill-in rule (:683-690) run for some instances and not for others."""
    labels = [11, 6060, 11, 5]
    ws = oracle.rand_fr_columns(200 + 7 * k + q, 1 << k, 4)
    got = prove_batch(hostcheck, tparams, cparams, 1, k, labels, ws, q)
    for b in range(4):
        assert got[b] == oracle.sumcheck_prove(1, k, labels[b], ws[b], q=q), b
    if k > 0:
        assert len(set(got)) == 4


@pytest.mark.parametrize("B", [1, 3, 17])
@pytest.mark.parametrize("n_in", [16, 37, 256, 5])
def test_ds_batch_level_equals_tree_by_tree(hostcheck, cparams, oracle, B, n_in):
    rng = random.Random(B * 1000 + n_in)
    labels = np.array([rng.choice([0, 3, 2025, 1 << 40]) for _ in range(B)], dtype=np.uint64)
    x = np.ascontiguousarray(oracle.rand_fr_columns(B + n_in, n_in, B).reshape(B * n_in, 4))
    per = (n_in + 15) // 16
    level, pos0 = 2, 48
    for by_ptrs in (0, 1):
        out = np.zeros((B * per, 4), np.uint64)
        assert hostcheck.l.hc_hash_ds_batch_level(cparams, C.c_size_t(16), C.c_uint32(level), C.c_uint64(pos0), ptr(labels), ptr(x), C.c_size_t(n_in),
                                                  C.c_size_t(B), by_ptrs, ptr(out)) == 0
        for b in range(B):
            want = np.zeros((per, 4), np.uint64)
            xb = np.ascontiguousarray(x[b * n_in:(b + 1) * n_in])
            assert hostcheck.l.hc_hash_ds_level(cparams, 0, C.c_size_t(16), C.c_uint32(level), C.c_uint64(pos0), C.c_uint64(int(labels[b])), ptr(xb), None,
                                                C.c_size_t(n_in), ptr(want)) == 0
            assert (out[b * per:(b + 1) * per] == want).all(), (by_ptrs, b)


class Model:
    """Transcript::new's state without a label, the lazy duplex, and a `finish` that permutes and squeezes (pure Python)."""
    def __init__(self):
        self.t = pyref.Transcript(b"")
        self.t.state = [0] * 16 + [pyref.tag_field(b"FSv1-TRANSCRIPT-INIT")]; self.t.pos = 0

    def absorb(self, xs):
        for x in xs:
            self.t.absorb_field(x)

    def finish(self):
        self.t.state = pyref.permute(self.t.state, self.t.P); self.t.pos = 0
        return self.t.state[0]


def tr_launch(hostcheck, tparams, state, pos, segs, pool0, pool1, inst=None, inst0=0, reset=0, finish_last=1):
    """segs[a] = list of nseg index lists for active a; returns out as canonical ints, shape (n_active, nseg)"""
    n_active, nseg = len(segs), len(segs[0])
    el_off, idx = [0], []
    for s in segs:
        assert len(s) == nseg
        for seg in s:
            idx += seg; el_off.append(len(idx))
    el_off = np.array(el_off, np.uint32); idx = np.array(idx or [0], np.uint32)
    ins = None if inst is None else np.array(inst, np.uint32)
    out = np.zeros((n_active * nseg, 4), np.uint64)
    n_inst = state.shape[0] // 17
    assert hostcheck.l.hc_tr_batch(tparams, ptr(state), ptr(pos), C.c_size_t(n_inst), None if ins is None else ptr(ins), C.c_size_t(inst0), C.c_size_t(n_active),
                                   C.c_size_t(nseg), ptr(el_off), ptr(idx), ptr(pool0), C.c_size_t(pool0.shape[0]), ptr(pool1), C.c_size_t(pool1.shape[0]),
                                   reset, finish_last, ptr(out)) == 0
    return [[pyref.from_limbs(out[a * nseg + s]) for s in range(nseg)] for a in range(n_active)]


def test_transcript_batch_stream_matches_reference(hostcheck, tparams):
    rng = random.Random(5)
    p = pyref.P_PALLAS
    v0 = [rng.randrange(p) for _ in range(60)]; v1 = [rng.randrange(p) for _ in range(20)]
    pool0 = np.array([pyref.to_limbs(x) for x in v0], np.uint64); pool1 = np.array([pyref.to_limbs(x) for x in v1], np.uint64)
    K1 = 0x80000000
    val = lambda i: v1[i & ~K1] if i & K1 else v0[i]
    n_inst = 4
    state = np.zeros((17 * n_inst, 4), np.uint64); pos = np.zeros(n_inst, np.uint32)
    models = [Model() for _ in range(n_inst)]
    # launch 1: every instance from Transcript::new, two segments of ragged lengths (0 .. 37 elements, across rate blocks), both pools
    segs = []
    for b in range(n_inst):
        a = [rng.randrange(60) for _ in range([3, 16, 17, 37][b])] + [K1 | rng.randrange(20) for _ in range(b)]
        c = [rng.randrange(60) for _ in range([0, 5, 16, 2][b])]
        segs.append([a, c])
    got = tr_launch(hostcheck, tparams, state, pos, segs, pool0, pool1, reset=1)
    for b in range(n_inst):
        for s in range(2):
            models[b].absorb([val(i) for i in segs[b][s]])
            assert got[b][s] == models[b].finish(), (b, s)
    assert (pos == 0).all()
    # launch 2: a subset absorbs without finishing — the cursors now differ per instance
    sub = [3, 1]
    segs2 = [[[rng.randrange(60) for _ in range(20)]], [[K1 | rng.randrange(20) for _ in range(5)]]]
    tr_launch(hostcheck, tparams, state, pos, segs2, pool0, pool1, inst=sub, finish_last=0)
    for a, b in enumerate(sub):
        models[b].absorb([val(i) for i in segs2[a][0]])
    assert list(pos) == [0, 5, 0, 4]
    assert [m.t.pos for m in models] == [0, 5, 0, 4]
    # launch 3: all instances again, three segments each; the stored cursors decide where the lazy permutations fall
    segs3 = [[[rng.randrange(60) for _ in range(rng.randrange(0, 30))] for _ in range(3)] for _ in range(n_inst)]
    got = tr_launch(hostcheck, tparams, state, pos, segs3, pool0, pool1)
    for b in range(n_inst):
        for s in range(3):
            models[b].absorb([val(i) for i in segs3[b][s]])
            assert got[b][s] == models[b].finish(), (b, s)
    # instances [2, 4) of a second batch through inst0, from reset: the first challenge equals Transcript::new(label) ... challenge(label)
    st2 = np.zeros((17 * 4, 4), np.uint64); pos2 = np.zeros(4, np.uint32)
    ab, ch = pyref.tag_field(b"FSv1-ABSORB-BYTES"), pyref.tag_field(b"FSv1-CHALLENGE")
    stream = [ab] + pyref.words(b"E2E/PLAIN") + [v0[7]] + [ch, ab] + pyref.words(b"c")
    pool = np.array([pyref.to_limbs(x) for x in stream], np.uint64)
    got = tr_launch(hostcheck, tparams, st2, pos2, [[list(range(len(stream)))]] * 2, pool, pool1, inst0=2, reset=1)
    t = pyref.Transcript(b"E2E/PLAIN"); t.absorb_field(v0[7]); want = t.challenge(b"c")
    assert got[0][0] == want and got[1][0] == want
    assert (st2[:34] == 0).all()
