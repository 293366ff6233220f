"""The mixed-size batch prove on the GPU: stark_tr_hash_many_dev (the Ragged layout of TrStream through the five-wave, one-wave and lane kernels)
and stark_deep_fri_prove_mixed_batch_dev (all column sponges in one ragged launch, then the equal-shape tails group by group).  Every digest
equals the oracle's and the single-item call's; every proof is byte-equal to deep_fri_prove of that trace alone.  The host twin of the ragged
hash and the grouping are tested in tests/test_mixed_prove_host.py.  Needs an MI355X: `pytest -m gpu`.

poseidon_form gives the ragged launch the form of the column sponges whatever the item count (five waves; one wave under "sponge_one_wave"), and
the lane form under "poseidon_lane_only": there is no count at which the form changes, so the counts are those of the host test (1, 4, 5, 70)
plus 130 — three workgroups of the lane form, the last one partly filled, as 70 leaves the second."""
import ctypes as C

import numpy as np
import pytest

import mixed_prove_cases as mp
from test_gpu_guard_bands import Band, PREFILLS

pytestmark = pytest.mark.gpu
vp = C.c_void_p
SEED_Z = 0xDEEFBAAD
INVALID_ARG = -1
OPTS = [None, ("sponge_one_wave", 1), ("poseidon_lane_only", 1)]
COUNTS = mp.COUNTS + (130,)


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.uint64).view(np.int64)).cuda()


def sync(ctx):
    ctx._chk(ctx.lib.stark_ctx_sync(ctx.h))


# ---- the ragged hash ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hash_refs(gpu_ctx, oracle, hostcheck):
    """count -> (items, the oracle's digests, the digests of stark_tr_hash_fields_tagged_dev on every item alone): made once, default options"""
    import torch
    pl = mp.pool(oracle); d = dev(pl); out = {}
    for count in COUNTS:
        items = mp.items_for(hostcheck, count)
        one = torch.zeros((count, 4), dtype=torch.int64, device="cuda")
        for i, (tag, off, k) in enumerate(items):
            gpu_ctx._chk(gpu_ctx.lib.stark_tr_hash_fields_tagged_dev(gpu_ctx.h, None, tag, vp(d.data_ptr() + 32 * off) if k else None, k, 1, vp(one.data_ptr() + 32 * i)))
        sync(gpu_ctx)
        out[count] = (items, mp.oracle_digests(oracle, pl, items), one.cpu().numpy().view(np.uint64))
    return pl, out


@pytest.mark.parametrize("opt", OPTS)
@pytest.mark.parametrize("count", COUNTS)
def test_tr_hash_many(gpu_ctx, hash_refs, count, opt):
    pl, refs = hash_refs
    items, want, single = refs[count]
    assert (want == single).all()
    inb = Band([pl])
    if opt:
        gpu_ctx.set_option(*opt)
    try:
        for pre in PREFILLS:
            ob = Band([count], prefill=pre)
            base = inb.ptr(0).value
            gpu_ctx.tr_hash_many_dev([(tag, base + 32 * off if k else None, k) for tag, off, k in items], ob.ptr(0).value)
            sync(gpu_ctx)
            got = ob.payload(0)
            bad = [i for i in range(count) if not (got[i] == want[i]).all()]
            assert not bad, (count, opt, pre, [(i, items[i]) for i in bad[:8]])
            ob.check("stark_tr_hash_many_dev out, n = %d, %s" % (count, opt))
            inb.check_unchanged("stark_tr_hash_many_dev fields, n = %d, %s" % (count, opt))
    finally:
        if opt:
            gpu_ctx.set_option(opt[0], 0)


def test_tr_hash_many_arguments(gpu_ctx, oracle):
    import torch
    lib, h = gpu_ctx.lib, gpu_ctx.h
    d = dev(mp.pool(oracle)); out = torch.full((4, 4), 0x5A, dtype=torch.int64, device="cuda")
    n = 3
    tags = (C.c_char_p * n)(*mp.TAGS[:n]); holed = (C.c_char_p * n)(mp.TAGS[0], None, mp.TAGS[2])
    ks = (C.c_size_t * n)(3, 0, 5); k0 = (C.c_size_t * n)(0, 0, 0)
    fl = (vp * n)(d.data_ptr(), None, d.data_ptr()); fl_bad = (vp * n)(d.data_ptr(), None, None)
    fl_over = (vp * n)(d.data_ptr(), None, out.data_ptr() + 32)         # the fields of item 2 lie inside out
    o = vp(out.data_ptr())
    assert lib.stark_tr_hash_many_dev(h, 0, None, None, None, None) == 0
    for args in [(None, n, tags, fl, ks, o), (h, n, None, fl, ks, o), (h, n, tags, fl, None, o), (h, n, tags, fl, ks, None), (h, n, holed, fl, ks, o),
                 (h, n, tags, None, ks, o), (h, n, tags, fl_bad, ks, o), (h, n, tags, fl_over, ks, o)]:
        assert lib.stark_tr_hash_many_dev(*args) == INVALID_ARG, args
    sync(gpu_ctx)
    assert (out.cpu().numpy() == 0x5A).all()                             # nothing was launched
    gpu_ctx._chk(lib.stark_tr_hash_many_dev(h, n, tags, None, k0, o))   # no fields at all: the table may be null
    sync(gpu_ctx)
    got = out.cpu().numpy().view(np.uint64)
    for i in range(n):
        assert (got[i] == oracle.tr_hash_fields_tagged(mp.TAGS[i], np.zeros((0, 4), np.uint64))).all(), i
    assert (got[3] == 0x5A).all()


# ---- the mixed prove ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mixed(gpu_ctx, oracle):
    """the seven traces of mp.PROVE_ORDER on the device, their shapes, and deep_fri_prove of each trace alone (default options): made once"""
    from stark_mlwe_amd.api import DeepFriParams
    host, devs, shapes, want = [], [], [], []
    for i, k in enumerate(mp.PROVE_ORDER):
        sched, r = mp.PROVE_SHAPES[k]; n0 = 1 << k
        cols = oracle.rand_fr_columns(0xB17C0 + i, n0, 4)
        host.append(cols); devs.append([dev(cols[c]) for c in range(4)]); shapes.append((n0, sched, r))
        want.append(gpu_ctx.deep_fri_prove(cols[0], cols[1], cols[2], cols[3], n0, DeepFriParams(sched, r, SEED_Z))[:2])
    return host, devs, shapes, want


def run_mixed(ctx, devs, shapes):
    return [g[:2] for g in ctx.deep_fri_prove_mixed_batch_dev([[c.data_ptr() for c in tr] for tr in devs], shapes, SEED_Z)]


def test_mixed_prove_equals_singles_and_oracle(gpu_ctx, oracle, mixed):
    host, devs, shapes, want = mixed
    before = [[c.cpu().numpy().copy() for c in tr] for tr in devs]
    got = run_mixed(gpu_ctx, devs, shapes)
    assert got == want
    assert len({g[0] for g in got}) == len(got)
    for i, k in enumerate(mp.PROVE_ORDER):
        if k <= 8:
            n0, sched, r = shapes[i]
            ref = oracle.deep_fri_prove(host[i][0], host[i][1], host[i][2], host[i][3], n0, sched, r, SEED_Z)
            assert got[i][0] == ref.bytes() and got[i][1] == ref.size_estimate(), i
            ref.free()
    for tr, b in zip(devs, before):
        for c, bc in zip(tr, b):
            assert (c.cpu().numpy() == bc).all()
    # stage times: every proof carries the sponge stage of the whole batch
    full = gpu_ctx.deep_fri_prove_mixed_batch_dev([[c.data_ptr() for c in tr] for tr in devs], shapes, SEED_Z)
    assert all(len(g[2]) == 3 and g[2][0] > 0 for g in full)
    # an equal-shape batch through the mixed call is the equal-shape batch
    idx = [i for i, k in enumerate(mp.PROVE_ORDER) if k == 6]
    assert run_mixed(gpu_ctx, [devs[i] for i in idx], [shapes[i] for i in idx]) == [want[i] for i in idx]
    assert run_mixed(gpu_ctx, [devs[1]], [shapes[1]]) == [want[1]]


def test_mixed_prove_in_passes_and_under_poison(gpu_ctx, mixed):
    """prove_batch_max_rows = 64 cuts the k = 6 group into passes of one trace; pool_poison 0x5A and 0x00: no result may depend on a stale block"""
    _, devs, shapes, want = mixed
    try:
        gpu_ctx.set_option("prove_batch_max_rows", 64)
        assert run_mixed(gpu_ctx, devs, shapes) == want
        gpu_ctx.set_option("prove_batch_max_rows", 1 << 22)
        for fill in (0x5A, 0x00):
            gpu_ctx.set_option("pool_poison", fill)
            assert run_mixed(gpu_ctx, devs, shapes) == want, fill
    finally:
        gpu_ctx.set_option("prove_batch_max_rows", 1 << 22)
        gpu_ctx.set_option("pool_poison", -1)


def test_reference_sweep_k11_to_k16_in_one_call(gpu_ctx, oracle):
    """The reference's bench inputs (end_to_end.rs:214, 229-253: seed chain from 1337, one LCG step per k from 11) for k = 11..16, schedule
    [16, 16, 8], r = 32, in ONE mixed call: the size estimates are the published ones (crates/channel/benchmarkdata.csv), the encoded lengths the
    oracle's (tests/golden/oracle_fingerprint_k11_k18.txt), and the oracle's verifier accepts the proofs of k <= 13."""
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
    got = run_mixed(gpu_ctx, devs, shapes)
    for k, (proof, e) in zip(range(11, 17), got):
        assert e == est[k], k
        assert len(proof) == lens[k], k
        if k <= 13:
            assert oracle.deep_fri_verify(proof, sched, r, SEED_Z) == 1, k


def test_mixed_prove_errors(gpu_ctx, mixed):
    """batch == 0; then one bad trace among good ones: INVALID_ARG, every out[i] NULL, nothing allocated, enqueued or leaked"""
    _, devs, shapes, want = mixed
    lib, h = gpu_ctx.lib, gpu_ctx.h
    B = len(devs)
    assert lib.stark_deep_fri_prove_mixed_batch_dev(h, 0, None, None, None, None, None, None, None, None, SEED_Z, None) == 0

    def call(n0s, scheds, holes=()):
        cols = [(vp * B)(*[None if (c, i) in holes else devs[i][c].data_ptr() for i in range(B)]) for c in range(4)]
        flat, off = [], [0]
        for s in scheds:
            flat += list(s); off.append(len(flat))
        n0 = (C.c_size_t * B)(*n0s); rr = (C.c_size_t * B)(*[s[2] for s in shapes])
        sch = (C.c_size_t * max(len(flat), 1))(*flat); offs = (C.c_size_t * (B + 1))(*off)
        out = (vp * B)(*[vp(0xDEAD)] * B)
        rc = lib.stark_deep_fri_prove_mixed_batch_dev(h, B, cols[0], cols[1], cols[2], cols[3], n0, sch, offs, rr, SEED_Z, out)
        return rc, [out[i] for i in range(B)]
    good_n0 = [s[0] for s in shapes]; good_sched = [s[1] for s in shapes]
    sync(gpu_ctx)
    cached = lib.stark_ctx_cached_bytes(h)
    bad_n0 = list(good_n0); bad_n0[3] = 24
    bad_sched = list(good_sched); bad_sched[1] = [16, 16, 8]                # 1024 / 256 = 4 is not divisible by 8
    for args in [(bad_n0, good_sched), (good_n0, good_sched, {(2, 4)}), (good_n0, bad_sched)]:
        rc, out = call(*args)
        assert rc == INVALID_ARG and out == [None] * B, args
        assert lib.stark_ctx_cached_bytes(h) == cached, args
    rc, out = call(good_n0, good_sched)                                     # the context stays usable
    assert rc == 0
    assert [g[:2] for g in gpu_ctx._proofs_out(out, B)] == want
