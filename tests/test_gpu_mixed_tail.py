"""The ragged prove tail on the GPU: stark_deep_fri_prove_mixed_batch_dev under the context option "mixed_prove_tail" = 1 — traces of one schedule and any
n0 and r share ONE merge (k_ali_merge_ragged), one commit phase (FriMixedCommit: k_zpows_many, k_fri_fold_ragged, DsRaggedPairStream, the ragged climb)
and one query phase.  Every proof is byte-equal to deep_fri_prove of that trace alone under default options (the unchanged single path).  The host twin
is tests/test_fri_mixed_host.py.  Needs an MI355X: `pytest -m gpu`."""
import ctypes as C

import numpy as np
import pytest

import fri_mixed_cases as fm

pytestmark = pytest.mark.gpu
vp = C.c_void_p
SEED_Z = fm.SEED_Z
INVALID_ARG = -1
ROWS_DEFAULT = 1 << 22


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.uint64).view(np.int64)).cuda()


def run_mixed(ctx, devs, shapes):
    return [g[:2] for g in ctx.deep_fri_prove_mixed_batch_dev([[c.data_ptr() for c in tr] for tr in devs], shapes, SEED_Z)]


class tail:
    """the option for the length of a with block; restored whatever happens"""
    def __init__(self, ctx, **more): self.ctx, self.more = ctx, more
    def __enter__(self):
        self.ctx.set_option("mixed_prove_tail", 1)
        for k, v in self.more.items():
            self.ctx.set_option(k, v)
    def __exit__(self, *a):
        self.ctx.set_option("mixed_prove_tail", -1)
        self.ctx.set_option("prove_batch_max_rows", ROWS_DEFAULT)
        self.ctx.set_option("pool_poison", -1)


@pytest.fixture(scope="module")
def twelve(gpu_ctx, oracle):
    """the twelve traces of fm.TRACES on the device and deep_fri_prove of each trace alone under default options: made once"""
    from stark_mlwe_amd.api import DeepFriParams
    host, devs, want = [], [], []
    for i, (n0, sched, r) in enumerate(fm.TRACES):
        cols = oracle.rand_fr_columns(0x7A11 + i, n0, 4)
        host.append(cols); devs.append([dev(cols[c]) for c in range(4)])
        want.append(gpu_ctx.deep_fri_prove(cols[0], cols[1], cols[2], cols[3], n0, DeepFriParams(sched, r, SEED_Z))[:2])
    return host, devs, want


def test_option_values(gpu_ctx):
    from stark_mlwe_amd.api import StarkError
    try:
        gpu_ctx.set_option("mixed_prove_tail", 1)
        gpu_ctx.set_option("mixed_prove_tail", 0)
        with pytest.raises(StarkError) as e:
            gpu_ctx.set_option("mixed_prove_tail", 2)
        assert e.value.code == INVALID_ARG and "mixed_prove_tail" in str(e.value)
        with pytest.raises(StarkError) as e:
            gpu_ctx.set_option("mixed_prove_tail", -2)
        assert e.value.code == INVALID_ARG
        gpu_ctx.set_option("mixed_prove_tail", 1)
        gpu_ctx.set_option("mixed_prove_tail", -1)                                   # the default
        with pytest.raises(StarkError) as e:
            gpu_ctx.set_option("no_such_option", 1)
        assert "mixed_prove_tail" in str(e.value)                                   # the known keys
    finally:
        gpu_ctx.set_option("mixed_prove_tail", -1)


def test_ragged_tail_equals_singles_and_oracle(gpu_ctx, oracle, twelve):
    host, devs, want = twelve
    before = [[c.cpu().numpy().copy() for c in tr] for tr in devs]
    with tail(gpu_ctx):
        got = run_mixed(gpu_ctx, devs, fm.TRACES)
        full = gpu_ctx.deep_fri_prove_mixed_batch_dev([[c.data_ptr() for c in tr] for tr in devs], fm.TRACES, SEED_Z)
        one_class = [i for i, c in enumerate(fm.CLASS_OF) if c == 1]
        sub = run_mixed(gpu_ctx, [devs[i] for i in one_class], [fm.TRACES[i] for i in one_class])
        alone = run_mixed(gpu_ctx, [devs[11]], [fm.TRACES[11]])
    bad = [i for i in range(len(want)) if got[i] != want[i]]
    assert not bad, [(i, fm.TRACES[i], got[i][1], want[i][1], len(got[i][0]), len(want[i][0])) for i in bad]
    assert len({g[0] for g in got}) == len(got)
    for i, (n0, sched, r) in enumerate(fm.TRACES):
        if n0 <= 1 << 8:
            ref = oracle.deep_fri_prove(host[i][0], host[i][1], host[i][2], host[i][3], n0, sched, r, SEED_Z)
            assert got[i][0] == ref.bytes() and got[i][1] == ref.size_estimate(), i
            ref.free()
    for tr, b in zip(devs, before):
        for c, bc in zip(tr, b):
            assert (c.cpu().numpy() == bc).all()
    # stage times: the pass's shared times, the sponge stage of the whole batch in [0]
    assert all(len(g[2]) == 3 and g[2][0] > 0 and g[2][1] >= 0 and g[2][2] > 0 for g in full)
    for cls in range(4):
        mine = [full[i][2] for i in range(len(full)) if fm.CLASS_OF[i] == cls]
        assert all(m == mine[0] for m in mine), cls                                  # one pass per class here
    assert sub == [want[i] for i in one_class] and alone == [want[11]]
    # the default is unchanged by all this
    assert run_mixed(gpu_ctx, devs[:3], fm.TRACES[:3]) == want[:3]


def test_ragged_tail_in_passes_and_under_poison(gpu_ctx, twelve):
    """prove_batch_max_rows = 5000 cuts the [16,8] class into {1}, {4, 7}, {10}, {11} and the [4,2] class into {0, 2, 6}, {9}; pool_poison 0x5A and 0x00:
    no result may depend on a stale block"""
    _, devs, want = twelve
    with tail(gpu_ctx, prove_batch_max_rows=fm.PASS_ROWS):
        assert run_mixed(gpu_ctx, devs, fm.TRACES) == want
    for fill in (0x5A, 0x00):
        with tail(gpu_ctx, pool_poison=fill):
            assert run_mixed(gpu_ctx, devs, fm.TRACES) == want, fill


def test_reference_sweep_k11_to_k16_under_the_ragged_tail(gpu_ctx, oracle):
    """the sweep of tests/test_gpu_mixed_prove.py (k = 11..16, [16, 16, 8], r = 32, the reference's bench inputs) as ONE class: the published size
    estimates, the oracle's encoded lengths, and the oracle's verifier accepts k <= 13"""
    import os
    sched, r = [16, 16, 8], 32
    est = {11: 39592, 12: 52000, 13: 60968, 14: 72936, 15: 87736, 16: 101976}
    lens = {12: 55633, 13: 64844, 14: 76973, 15: 91998, 16: 106420}
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "oracle_fingerprint_k11_k18.txt")
    for line in open(gold):
        f = line.split(",")
        if f[1] == "11":
            assert int(f[2]) == est[11]; lens[11] = int(f[3])
    devs, shapes, seed = [], [], 1337
    for k in range(11, 17):
        seed = (seed * 1103515245 + 12345) % 2**64
        cols = oracle.rand_fr_columns(seed, 1 << k, 4)
        devs.append([dev(cols[c]) for c in range(4)]); shapes.append((1 << k, sched, r))
    with tail(gpu_ctx):
        got = run_mixed(gpu_ctx, devs, shapes)
    for k, (proof, e) in zip(range(11, 17), got):
        assert e == est[k], k
        assert len(proof) == lens[k], k
        if k <= 13:
            assert oracle.deep_fri_verify(proof, sched, r, SEED_Z) == 1, k


def test_errors_under_the_ragged_tail(gpu_ctx, twelve):
    """one bad trace among good ones: INVALID_ARG, every out[i] NULL, the pool's cached bytes unchanged; the context stays usable"""
    _, devs, want = twelve
    lib, h = gpu_ctx.lib, gpu_ctx.h
    use = [0, 1, 2, 4, 6, 7, 9]; B = len(use)
    shapes = [fm.TRACES[i] for i in use]

    def call(n0s, scheds, holes=()):
        cols = [(vp * B)(*[None if (c, j) in holes else devs[i][c].data_ptr() for j, i in enumerate(use)]) for c in range(4)]
        sch, offs = fm.flat_schedules(scheds)
        n0 = (C.c_size_t * B)(*n0s); rr = (C.c_size_t * B)(*[s[2] for s in shapes])
        out = (vp * B)(*[vp(0xDEAD)] * B)
        rc = lib.stark_deep_fri_prove_mixed_batch_dev(h, B, cols[0], cols[1], cols[2], cols[3], n0, sch, offs, rr, SEED_Z, out)
        return rc, [out[j] for j in range(B)]
    good_n0 = [s[0] for s in shapes]; good_sched = [s[1] for s in shapes]
    with tail(gpu_ctx):
        assert lib.stark_deep_fri_prove_mixed_batch_dev(h, 0, None, None, None, None, None, None, None, None, SEED_Z, None) == 0
        gpu_ctx.sync()
        cached = lib.stark_ctx_cached_bytes(h)
        bad_n0 = list(good_n0); bad_n0[3] = 24
        bad_sched = list(good_sched); bad_sched[1] = [16, 16, 8]                    # 1024 / 256 = 4 is not divisible by 8
        for args in [(bad_n0, good_sched), (good_n0, good_sched, {(2, 4)}), (good_n0, bad_sched)]:
            rc, out = call(*args)
            assert rc == INVALID_ARG and out == [None] * B, args
            assert lib.stark_ctx_cached_bytes(h) == cached, args
        rc, out = call(good_n0, good_sched)                                         # the context stays usable
        assert rc == 0
        assert [g[:2] for g in gpu_ctx._proofs_out(out, B)] == [want[i] for i in use]


def test_fewer_allocation_requests(gpu_ctx, oracle):
    """six traces of six sizes in one class: under option 0 six single tails, under option 1 one ragged pass — strictly fewer allocation requests"""
    sched, r = [4, 2], 4
    devs, shapes = [], []
    for k in range(6, 12):
        cols = oracle.rand_fr_columns(0xA110C + k, 1 << k, 4)
        devs.append([dev(cols[c]) for c in range(4)]); shapes.append((1 << k, sched, r))
    counts = {}
    try:
        for opt in (0, 1):
            gpu_ctx.set_option("mixed_prove_tail", opt)
            counts[("warm", opt)] = run_mixed(gpu_ctx, devs, shapes)                 # constants and challenges cached: the counted call allocates for the call alone
            gpu_ctx.diag_alloc_refusal(1, 0)
            got = run_mixed(gpu_ctx, devs, shapes)
            counts[opt] = gpu_ctx.diag_alloc_refusal(-1)[0]
            gpu_ctx.diag_alloc_refusal(0, 0)
            assert got == counts[("warm", opt)]
    finally:
        gpu_ctx.diag_alloc_refusal(0, 0)
        gpu_ctx.set_option("mixed_prove_tail", -1)
    assert counts[("warm", 0)] == counts[("warm", 1)]
    print("allocation requests: option 0 %d, option 1 %d" % (counts[0], counts[1]))
    assert 0 < counts[1] < counts[0], counts
