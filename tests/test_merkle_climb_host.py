"""The two Merkle climbs of csrc/merkle_batch.hpp (merkle_climb, merkle_climb_ragged) on the CPU, without a hash compared: the ragged plan as data
(hc_merkle_ragged_plan) against the definition written out here, and the DS launches of the five call sites — merkle_build_batch,
merkle_build_mixed_batch, FriBatchCommit::run, ScBatch::commit_layers, ScBatch::commit_witnesses — recorded by the host executors (hc_climb_launches)
against lists derived from the shapes alone.  The expected lists are the loops each call site had of its own before the climb was written once; what
the hashes are is the matter of test_merkle_batch_host, test_mixed_batch_host, test_fri_batch_host and test_sumcheck_batch_host."""
import ctypes as C
import random

import numpy as np
import pytest

from hostcheck_lib import P

LENGTHS = (1, 2, 15, 16, 17, 32, 33, 256, 257)
ARITIES = (2, 4, 8, 16)
PAIR_LEVEL = 0xFFFFFFFF
PITCH, PTRS, PAIRS, RAGGED, RAGGED_PAIRS, PAIR_PTRS = 1, 2, 3, 4, 5, 6      # the stream kinds of hc_climb_launches


def level_lens(n, arity):
    """merkle/src/lib.rs:166-190: a level of `len` nodes has ceil(len / arity) parents, until one node is left"""
    lens = [n]
    while lens[-1] > 1:
        lens.append(-(-lens[-1] // arity))
    return lens


def batches():
    """equal batches of every length and mixed batches of 1 to 6 trees drawn from LENGTHS (fixed seed), each once"""
    rnd = random.Random(0xC11B); out = []
    for B in range(1, 7):
        out += [[n] * B for n in LENGTHS if B in (1, 3, 6) or n in (1, 17)]
        out += [[rnd.choice(LENGTHS) for _ in range(B)] for _ in range(6)]
    out += [[1, 257, 1, 16, 2, 1], [257, 256, 33, 32, 17, 16], [1, 1, 2]]
    return out


def plan_by_definition(arity, ns, labels, leaf_table):
    """-> (lens[b], at[b], block[v], tables[v] = [(first, n_in, label, tree)]): level v of the call is the slices of the trees with more than v levels
    in tree order; table v >= 1 is the launch that writes it, one segment per such tree, reading that tree's level v - 1; table 0 makes the leaves"""
    lens = [level_lens(n, arity) for n in ns]; depth = max(len(l) for l in lens)
    at = [[0] * len(l) for l in lens]; block = [0] * depth; tables = [[] for _ in range(depth)]
    for v in range(depth):
        for b, l in enumerate(lens):
            if len(l) > v:
                at[b][v] = block[v]; block[v] += l[v]
        first = 0
        for b, l in enumerate(lens):
            if len(l) > v and (v or leaf_table):
                tables[v].append((first, l[v - 1] if v else ns[b], labels[b], b)); first += l[v]
    return lens, at, block, tables


def hc_plan(hostcheck, arity, ns, labels, leaf_table):
    B = len(ns); n = np.array(ns, np.uint64); lab = np.array(labels, np.uint64); cap = 64 * B + B
    depth = C.c_size_t(0); nlev = np.zeros(B, np.uint64); lens = np.zeros(64 * B, np.uint64); at = np.zeros(64 * B, np.uint64)
    block, t0, n_seg, n_out = (np.zeros(64, np.uint64) for _ in range(4))
    first, n_in, label = (np.zeros(cap, np.uint64) for _ in range(3)); tree = np.zeros(cap, np.uint32)
    hostcheck.l.hc_merkle_ragged_plan.restype = C.c_long
    S = hostcheck.l.hc_merkle_ragged_plan(C.c_size_t(arity), C.c_size_t(B), P(n), P(lab), 1 if leaf_table else 0, C.byref(depth), P(nlev), P(lens), P(at),
                                          P(block), P(t0), P(n_seg), P(n_out), P(first), P(n_in), P(label), P(tree), C.c_size_t(cap))
    if S < 0:
        return None
    assert S <= cap
    d = depth.value
    got_lens = [[int(x) for x in lens[64 * b:64 * b + int(nlev[b])]] for b in range(B)]
    got_at = [[int(x) for x in at[64 * b:64 * b + int(nlev[b])]] for b in range(B)]
    tables = []
    for v in range(d):
        a, k = int(t0[v]), int(n_seg[v])
        tables.append([(int(first[s]), int(n_in[s]), int(label[s]), int(tree[s])) for s in range(a, a + k)])
    assert sum(len(t) for t in tables) == S and [int(x) for x in t0[:d]] == [sum(len(t) for t in tables[:v]) for v in range(d)]     # ONE table, back to back
    return got_lens, got_at, [int(x) for x in block[:d]], tables, [int(x) for x in n_out[:d]]


@pytest.mark.parametrize("arity", ARITIES)
def test_ragged_plan_equals_the_definition(hostcheck, arity):
    """lengths per tree, offsets per level, block sizes and every segment table (first, n_in, label, tree), with and without the leaves' table"""
    for ns in batches():
        labels = [1000 + 7 * b for b in range(len(ns))]
        for leaf_table in (True, False):
            lens, at, block, tables = plan_by_definition(arity, ns, labels, leaf_table)
            got = hc_plan(hostcheck, arity, ns, labels, leaf_table)
            assert got is not None, (arity, ns)
            assert got[0] == lens and got[1] == at and got[2] == block, (arity, ns, leaf_table)
            assert got[3] == tables, (arity, ns, leaf_table)
            assert got[4] == [block[v] if tables[v] else 0 for v in range(len(block))], (arity, ns, leaf_table)      # a launch writes its whole block


def test_ragged_plan_refuses_what_has_no_tree(hostcheck):
    assert hc_plan(hostcheck, 16, [4, 0], [1, 2], True) is None and hc_plan(hostcheck, 1, [2], [1], True) is None
    assert hc_plan(hostcheck, 1, [1, 1], [1, 2], True)[0] == [[1], [1]]


def launches(hostcheck, site, arity, ns, flag=0, schedule=()):
    n = np.array(ns, np.uint64); sch = np.array(list(schedule) or [0], np.uint64); cap = 512; out = np.zeros(4 * cap, np.int64)
    B = len(ns)
    hostcheck.l.hc_climb_launches.restype = C.c_long
    k = hostcheck.l.hc_climb_launches(site, C.c_size_t(arity), C.c_size_t(B), P(n), flag, P(sch), C.c_size_t(len(schedule)), P(out), C.c_size_t(cap))
    assert 0 <= k <= cap, (site, arity, ns, flag, schedule, k)
    return [tuple(int(x) for x in out[4 * i:4 * i + 4]) for i in range(k)]


def same_shape_levels(arity, n, B, first_kind, tops):
    """one DsBatchStream launch per level over all B trees: level number v - 1, B x lens[v] hashes; the last one into the top slots when there are any"""
    lens = level_lens(n, arity)
    return [(first_kind if v == 1 else PITCH, v - 1, B * lens[v], 1 if tops and v + 1 == len(lens) else 0) for v in range(1, len(lens))]


def ragged_levels(arity, ns, tops):
    """one DsRaggedStream launch per level over the trees that still have it"""
    lens = [level_lens(n, arity) for n in ns]; depth = max(len(l) for l in lens)
    return [(RAGGED, v - 1, sum(l[v] for l in lens if len(l) > v), 1 if tops and v + 1 == depth else 0) for v in range(1, depth)]


@pytest.mark.parametrize("arity", ARITIES)
def test_merkle_builds_launch_what_they_did(hostcheck, arity):
    """merkle_build_batch: the pair leaves (pairs) as one DsBatchPairPtrStream launch, then one DsBatchStream launch per level at a pitch, no top slots;
    merkle_build_mixed_batch: the same with the ragged stream over the trees that still have the level"""
    for B in (1, 3):
        for n in LENGTHS:
            for pairs in (0, 1):
                want = ([(PAIR_PTRS, PAIR_LEVEL, B * n, 0)] if pairs else []) + same_shape_levels(arity, n, B, PITCH, False)
                assert launches(hostcheck, 0, arity, [n] * B, pairs) == want, (arity, B, n, pairs)
    for ns in batches():
        for pairs in (0, 1):
            want = ([(RAGGED_PAIRS, PAIR_LEVEL, sum(ns), 0)] if pairs else []) + ragged_levels(arity, ns, False)
            assert launches(hostcheck, 1, arity, ns, pairs) == want, (arity, ns, pairs)


def pick_arity(n, m):                                                     # fri.rs:220-229
    for a in (128, 64, 32, 16, 8, 4):
        if m >= a and n % a == 0:
            return a
    return 2 if n % 2 == 0 else 1


@pytest.mark.parametrize("n0, schedule", [(64, (4, 2)), (32, (16,)), (16, (8,)), (36, (2,)), (256, (16, 8)), (24, (4,)), (8, (2, 2, 2))])
def test_fri_commit_launches_what_it_did(hostcheck, n0, schedule):
    """FriBatchCommit::run: the layers L .. 1, then layer 0; a hashed arity has its leaves from leaf_pairs (no DS launch), an unhashed one from one
    DsBatchPairStream launch; then one DsBatchStream launch per level, the top one into the roots — as are the leaves of a layer of one element"""
    for B in (1, 3):
        n = [n0]
        for m in schedule:
            n.append(n[-1] // m)
        L = len(schedule); want = []
        for l in list(range(L, 0, -1)) + [0]:
            a = pick_arity(n[l], schedule[l] if l < L else 1)
            if a not in (128, 64, 32, 16, 8):
                want.append((PAIRS, PAIR_LEVEL, B * n[l], 1 if n[l] == 1 else 0))
            want += same_shape_levels(a, n[l], B, PITCH, True)
        assert launches(hostcheck, 2, 16, [n0] * B, 0, schedule) == want, (B, n0, schedule)


def test_sumcheck_commits_launch_what_they_did(hostcheck):
    """ScBatch::commit_layers: arity 16, level 0 read in place (behind a pointer table or at a pitch), the top level into the root slots, a layer of one
    element no launch at all; commit_witnesses: witnesses of one size are commit_layers behind the witness table, of several sizes one ragged launch
    per level (the order of the trees does not change a level's hash count), the top one into the root slots"""
    for B in (1, 3):
        for n in (1, 2, 16, 32, 256, 512, 8192):
            for ptrs in (0, 1):
                assert launches(hostcheck, 3, 16, [n] * B, ptrs) == same_shape_levels(16, n, B, PTRS if ptrs else PITCH, True), (B, n, ptrs)
            assert launches(hostcheck, 4, 16, [n] * B) == same_shape_levels(16, n, B, PTRS, True), (B, n)
    for ns in ([1, 2], [2, 1, 16], [16, 32, 512, 1, 2], [512, 512, 16], [1, 1, 8192, 256], [32, 1, 32, 1, 2, 2]):
        assert launches(hostcheck, 4, 16, ns) == ragged_levels(16, ns, True), ns
