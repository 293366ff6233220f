"""The one layer-shape function (stark_mlwe_amd/csrc/fri_plan.hpp: fri_layers) on the CPU, through its two users in the host-check library: the query
plan (FriShape::make behind hc_fri_plan_create) and the batched commit (FriBatchCommit::shape behind hc_fri_commit_batch).  An empty layer, a
schedule that does not divide and a layer with arity 1 are refused, each user with its own code, before anything is hashed.  The arity-1 plans
are the regression: FriShape::make used to build the level lengths of such a layer first, a loop that does not end."""
import ctypes as C

import numpy as np
import pytest

vp = C.c_void_p
# (n0, schedule) -> the batched commit's return code (-1: empty or not dividing, -2: arity 1); the plan refuses every one of them
REFUSED = [(0, [], -1), (64, [16, 8], -1), (64, [1], -1), (3, [], -2), (6, [2], -2)]


def ptr(a):
    return a.ctypes.data_as(vp)


@pytest.fixture(scope="module")
def tparams(hostcheck):
    h = hostcheck.params(1)
    yield h
    hostcheck.params_free(h)


@pytest.mark.parametrize("n0,sched,commit_rc", REFUSED)
def test_refused_shapes(hostcheck, tparams, n0, sched, commit_rc):
    L = len(sched); sch = np.ascontiguousarray(sched if sched else [0], dtype=np.uint64)
    roots = np.zeros((2, L + 1, 4), np.uint64)
    hostcheck.l.hc_fri_plan_create.restype = vp
    assert hostcheck.l.hc_fri_plan_create(tparams, ptr(roots), C.c_size_t(n0), ptr(sch), C.c_size_t(L), C.c_size_t(4)) is None
    f = [np.zeros((max(n0, 1), 4), np.uint64) for _ in range(2)]
    tab = (vp * 2)(*[ptr(x) for x in f])
    assert hostcheck.l.hc_fri_commit_batch(tparams, C.c_size_t(2), tab, C.c_size_t(n0), ptr(sch), C.c_size_t(L), C.c_uint64(7), ptr(roots)) == commit_rc


def test_accepted_shape_still_plans(hostcheck, tparams):
    """arity 1 with ONE leaf is a tree of one node and stays accepted: 2 -> 1 under [2]"""
    roots = np.zeros((2, 4), np.uint64)
    plan = hostcheck.fri_plan(tparams, roots, 2, [2], 1)
    assert len(plan.requests()[0]) > 0
    hostcheck.l.hc_fri_plan_free(plan.h)
