"""The host side of the ragged prove tail (option "mixed_prove_tail"): FriMixedCommit (stark_mlwe_amd/csrc/fri_mixed.hpp) over the host executor against the
oracle's roots, the new pair-leaf stream and the ragged fold on their own, the classes and passes, and the driver's census.  No GPU needed; the device
side is tests/test_gpu_mixed_tail.py."""
import numpy as np
import pytest

import fri_mixed_cases as fm


@pytest.fixture(scope="module")
def tp(hostcheck):
    return hostcheck.params(1)


@pytest.fixture(scope="module")
def class_refs(oracle):
    """per class of fm.HOST_CLASSES: the layers f0 of its traces and the oracle's roots of deep_fri_prove(f0=) on each trace alone (made once, never changed)"""
    out = []
    for ci, (sched, sizes) in enumerate(fm.HOST_CLASSES):
        f0s, roots = [], []
        for i, n0 in enumerate(sizes):
            f0 = oracle.rand_fr_columns(0xF0F0 + 16 * ci + i, n0, 1)[0]
            ref = oracle.deep_fri_prove(None, None, None, None, n0, sched, 2, fm.SEED_Z, f0=f0)
            assert ref.num_layers() == len(sched) + 1
            f0s.append(f0); roots.append(np.stack([ref.root(l) for l in range(len(sched) + 1)])); ref.free()
        out.append((sched, f0s, roots))
    return out


@pytest.mark.parametrize("ci", range(len(fm.HOST_CLASSES)))
def test_roots_against_the_oracle(hostcheck, tp, class_refs, ci):
    sched, f0s, want = class_refs[ci]
    before = [f.copy() for f in f0s]
    got = fm.commit_mixed(hostcheck, tp, f0s, sched)
    for b in range(len(f0s)):
        assert (got[b] == want[b]).all(), (sched, b)
    rev = fm.commit_mixed(hostcheck, tp, f0s[::-1], sched)                          # the trace order reversed
    for b in range(len(f0s)):
        assert (rev[len(f0s) - 1 - b] == want[b]).all(), (sched, b)
    for b in range(len(f0s)):                                                       # B = 1
        assert (fm.commit_mixed(hostcheck, tp, [f0s[b]], sched)[0] == want[b]).all(), (sched, b)
    assert all((f == g).all() for f, g in zip(f0s, before))


@pytest.mark.parametrize("with_partners", [False, True])
@pytest.mark.parametrize("cp_div", [1, 2, 4])
def test_ragged_pair_stream_against_the_single_level(hostcheck, oracle, cp_div, with_partners):
    """trees of 1, 2, 12 and 64 leaves in one launch: tree by tree what hc_hash_ds_level mode 1 gives on that tree, with the partner of the launch's hash k
    at k / cp_div of the one partner array"""
    lens, arity = [1, 2, 12, 64], 4
    params = hostcheck.params(0, t=9)
    segs = [oracle.rand_fr_columns(0xAB00 + i, n, 1)[0] for i, n in enumerate(lens)]
    labels = [5, 5, 9, 2]
    total = sum(lens)
    in1 = oracle.rand_fr_columns(0xAB99, (total + cp_div - 1) // cp_div, 1)[0] if with_partners else None
    got = fm.ragged_pairs_level(hostcheck, params, arity, labels, segs, in1, cp_div)
    first = 0
    for s, n in enumerate(lens):
        part = None if in1 is None else np.stack([in1[(first + j) // cp_div] for j in range(n)])
        want = hostcheck.hash_ds_level(params, 1, arity, 0xFFFFFFFF, 0, labels[s], segs[s], part)
        assert (got[first:first + n] == want).all(), (cp_div, with_partners, s)
        first += n
    if with_partners:                                                               # no partners is the zero column, not an absent term
        zero = fm.ragged_pairs_level(hostcheck, params, arity, labels, segs, np.zeros_like(in1), cp_div)
        assert (zero == fm.ragged_pairs_level(hostcheck, params, arity, labels, segs, None, cp_div)).all()


@pytest.mark.parametrize("m", [2, 4, 16])
def test_ragged_fold_against_the_per_trace_fold(hostcheck, oracle, m):
    """segments of 1, 2 and 33 outputs, then one more that shares the first one's z: per segment what fri_fold_layer gives on that slice"""
    outs = [1, 2, 33, 2]
    zs = [oracle.rand_fr_columns(0x2200 + i, 1, 1)[0][0] for i in range(3)]
    zidx = [0, 1, 2, 0]
    zp = []
    for z in zs:
        acc = oracle.from_u64(1)
        for _ in range(m):
            zp.append(acc); acc = oracle.mul(acc, z)
    zp = np.stack(zp)
    f = oracle.rand_fr_columns(0x2299, sum(outs) * m, 1)[0]
    first, o = [], 0
    for k in outs:
        first.append(o); o += k
    got = fm.fold_ragged(hostcheck, f, first, [m * zi for zi in zidx], zp, m)
    for s, k in enumerate(outs):
        want = oracle.fri_fold_layer(f[first[s] * m:(first[s] + k) * m], zs[zidx[s]], m)
        assert (got[first[s]:first[s] + k] == want).all(), (m, s)
    # one segment is the plain fold
    assert (fm.fold_ragged(hostcheck, f, [0], [m], zp, m) == oracle.fri_fold_layer(f, zs[1], m)).all()


def test_classes_and_passes(hostcheck):
    cls, order, nc = fm.classes_of(hostcheck, fm.TRACES)
    assert nc == 4 and cls == fm.CLASS_OF and order == fm.CLASS_ORDER
    # n0 and r are free; another schedule length or entry is another class; the empty schedule is a class like any other
    shapes = [(64, [4, 2], 4), (128, [4, 2], 8), (64, [2, 4], 4), (64, [4], 4), (64, [], 4), (2, [], 1)]
    assert fm.classes_of(hostcheck, shapes) == ([0, 0, 1, 2, 3, 3], [0, 1, 2, 3, 4, 5], 4)
    assert fm.classes_of(hostcheck, [(64, [4, 2], 4)]) == ([0], [0], 1)
    big = [fm.TRACES[i][0] for i in order if cls[i] == 1]
    assert big == [1024, 4096, 128, 1024, 8192]
    assert fm.passes_of(hostcheck, big, fm.PASS_ROWS) == [1, 2, 1, 1]              # {1}, {4, 7}, {10}, {11}
    assert fm.passes_of(hostcheck, big, 1 << 22) == [5]
    assert fm.passes_of(hostcheck, big, 1) == [1] * 5                               # a pass always holds a trace
    assert fm.passes_of(hostcheck, big, 1 << 22, max_traces=2) == [2, 2, 1]
    assert fm.passes_of(hostcheck, [64] * 7, 200) == [3, 3, 1]                      # equal sizes: max_rows / n0 traces a pass, the equal-shape rule


def test_census_does_not_grow_with_the_traces(hostcheck):
    sched, sizes = [16, 8], [128, 1024, 4096]
    one = fm.commit_steps(hostcheck, sizes, sched)
    three = fm.commit_steps(hostcheck, [n for n in sizes for _ in range(3)], sched)
    assert one == three
    L = len(sched)
    assert one["folds"] == L and one["zpows"] == 1 and one["gathers"] == 1
    # per layer and arity part: one leaf launch, and one level launch per level of the part's largest tree above its leaves
    want_levels = want_hashed = want_pairs = 0
    for l in range(L + 1):
        m = sched[l] if l < L else 1
        parts = {}
        for n0 in sizes:
            n = fm.layer_sizes(n0, sched)[l]; a = fm.pick_arity(n, m)
            parts[a] = max(parts.get(a, 0), fm.tree_levels(n, a))
        for a, depth in parts.items():
            want_levels += depth - 1
            if a >= 8:
                want_hashed += 1
            else:
                want_pairs += 1
    assert (one["levels"], one["leaf_pairs"], one["pair_streams"]) == (want_levels, want_hashed, want_pairs)
    assert want_pairs == 2                                                          # the last layer: an arity-2 part (8 and 32 leaves) and the one-element layer of 128
    # a class of one size takes the plain fold and the same number of steps
    same = fm.commit_steps(hostcheck, [1024] * 4, sched)
    assert same["folds"] == L and same["blocks"] <= one["blocks"]
