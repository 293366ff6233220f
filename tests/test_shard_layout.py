"""The shard planner of the sharded commit phase (stark_fri_shard_layout, host-only product code) against the rules of dist.py's DistProver
(`_shardable`, `sharded_stop_len`), and the exports of the sharded FRI entry points.  CPU only."""
import ctypes as C

import numpy as np
import pytest

SCHEDULES = [[16, 16, 8], [8, 8, 8], [16, 8], [32, 32, 16], [64, 32, 8], [64, 64, 8, 2]]
NEW_SYMBOLS = ["stark_fri_build_sharded_dev", "stark_fri_shard_num_layers", "stark_fri_shard_root", "stark_fri_shard_is_sharded", "stark_fri_shard_free",
               "stark_fri_shard_prove_queries", "stark_deep_fri_prove_sharded_dev", "stark_diag_fri_build_sharded_emulated_dev",
               "stark_diag_deep_fri_prove_sharded_emulated_dev", "stark_fri_shard_layout"]


def _layout(n0, schedule, W):
    from stark_mlwe_amd._abi import load_library
    lib = load_library()
    sch = np.ascontiguousarray(schedule, dtype=np.uint64)
    sharded = np.full(len(sch) + 1, -7, np.int32); stop = np.zeros(len(sch) + 1, np.uint64)
    rc = lib.stark_fri_shard_layout(n0, sch.ctypes.data_as(C.c_void_p), len(sch), W, sharded.ctypes.data_as(C.c_void_p), stop.ctypes.data_as(C.c_void_p))
    return rc, [int(x) for x in sharded], [int(x) for x in stop]


def _divides(n0, schedule):
    n = n0
    for m in schedule:
        if m < 2 or n % m:
            return False
        n //= m
    return True


def _dist_rules(n0, schedule, W):
    """DistProver.commit's walk over the layers, with DistProver._shardable and dist.sharded_stop_len themselves."""
    from stark_mlwe_amd import dist
    pr = object.__new__(dist.DistProver)          # _shardable reads only W and the schedule: no process group needed
    pr.W, pr.schedule = W, list(schedule)
    L, n, prev = len(schedule), n0, True
    sharded, stop = [], []
    for l in range(L + 1):
        m = schedule[l] if l < L else 1
        now = pr._shardable(l, n, prev)
        sharded.append(int(now))
        stop.append(dist.sharded_stop_len(n // W, dist.pick_arity_for_layer(n, m)) if now else 1)
        prev = now
        if l < L:
            n //= m
    return sharded, stop


def test_library_exports_the_sharded_fri_entry_points():
    from stark_mlwe_amd._abi import load_library, SIGNATURES
    lib = load_library()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s), s
        assert s in SIGNATURES, s


@pytest.mark.parametrize("schedule", SCHEDULES, ids=lambda s: "x".join(map(str, s)))
def test_layout_follows_the_distprover_rules(schedule):
    """Every n0 = 2^7 .. 2^24 and W in {1, 2, 4, 8}: the library's plan is DistProver's (sharded flags and the local stop length of every lower
    tree); a schedule that does not divide n0 is refused."""
    checked = 0
    for k in range(7, 25):
        n0 = 1 << k
        for W in (1, 2, 4, 8):
            rc, sharded, stop = _layout(n0, schedule, W)
            if not _divides(n0, schedule):
                assert rc == -1, (n0, schedule, W)
                continue
            assert rc == 0, (n0, schedule, W)
            assert (sharded, stop) == _dist_rules(n0, schedule, W), (n0, schedule, W)
            checked += 1
    assert checked > 0


def test_layout_sharded_layers_change_with_the_rank_count():
    """[16,16,8] at 2^12: layer 2 (16 elements) is sharded up to W = 2, replicated at W = 8 (2 elements per rank hold no group of 8)."""
    _, s1, _ = _layout(1 << 12, [16, 16, 8], 1)
    _, s8, _ = _layout(1 << 12, [16, 16, 8], 8)
    assert s1[:3] == [1, 1, 1] and s8[:3] == [1, 1, 0]


@pytest.mark.parametrize("n0,W", [(1 << 12, 3), (1 << 12, 0), (1 << 12, -2), (1 << 12, 6), (4, 8), (20, 8)])
def test_layout_refuses_bad_rank_counts(n0, W):
    rc, _, _ = _layout(n0, [2], W)
    assert rc == -1


def test_layout_python_helper():
    from stark_mlwe_amd.api import fri_shard_layout, StarkError
    sharded, stop = fri_shard_layout(1 << 20, [16, 16, 8], 8)
    assert sharded == [True, True, True, False] and stop == [2, 2, 1, 1]      # the last layer commits pairs (arity 2): replicated
    with pytest.raises(StarkError):
        fri_shard_layout(1 << 20, [16, 16, 8], 3)
