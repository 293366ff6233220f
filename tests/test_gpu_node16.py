"""The arity-16 node kernel (poseidon_pair.hpp k_node16_pair) and the wave-pair form of the side stream's commitments (capi_fri.hip fri_build_impl).
Option "merkle_node16_pair" = 0 keeps the generic wave-pair kernel k_hash_ds2<17>, option "fri_side_pair" = 0 the latency forms on the side
stream: same values every way, and the oracle's hash_with_ds_dynamic on sampled nodes.  Needs an MI355X: `pytest -m gpu`."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _with_option(ctx, key, value, fn):
    ctx._chk(ctx.lib.stark_ctx_set_option(ctx.h, key, value))
    try:
        return fn()
    finally:
        ctx._chk(ctx.lib.stark_ctx_set_option(ctx.h, key, 1))


@pytest.mark.parametrize("nodes,level,label", [(4096, 0, 0), (4097, 3, 42), (8192, 1, 7), (8193, 2, 5), (1 << 15, 5, 0xFFFFFFFF), (1 << 15, 0, 1)])
def test_node16_level_equals_generic_kernel_and_oracle(gpu_ctx, oracle, nodes, level, label):
    """One Merkle level of `nodes` nodes with 16 children each, DS positions from 1000: the new kernel (from 4097 nodes on) against k_hash_ds2<17>
    (option off) on every node, and against the oracle's hash_with_ds_dynamic on sampled nodes.  4096 nodes run the one-wave kernel either way."""
    p17 = gpu_ctx.poseidon_params_for_width(17)
    ch = oracle.synth_column(700 + nodes + level, 3, 0, nodes * 16)
    got = gpu_ctx.hash_ds_level(p17, 16, level, 1000, label, ch)
    assert got.shape[0] == nodes
    old = _with_option(gpu_ctx, b"merkle_node16_pair", 0, lambda: gpu_ctx.hash_ds_level(p17, 16, level, 1000, label, ch))
    assert (got == old).all()
    fe = lambda x: oracle.from_u64(x)
    for k in sorted({0, 1, 63, 64, nodes // 2, nodes - 2, nodes - 1}):
        kids = ch[16 * k: 16 * k + 16]
        ds = np.array([fe(16), fe(level), fe(1000 + k), fe(label)])
        assert (got[k] == oracle.hash_with_ds_dynamic(0, 17, ds, kids, 16)).all(), k


def test_ragged_level_keeps_generic_kernel(gpu_ctx, oracle):
    """A level of more than 4096 nodes whose last node is ragged is not the new kernel's: its values equal the option-off run and the oracle."""
    p17 = gpu_ctx.poseidon_params_for_width(17)
    n_in = 8192 * 16 + 5
    ch = oracle.synth_column(811, 4, 0, n_in)
    got = gpu_ctx.hash_ds_level(p17, 16, 2, 0, 9, ch)
    old = _with_option(gpu_ctx, b"merkle_node16_pair", 0, lambda: gpu_ctx.hash_ds_level(p17, 16, 2, 0, 9, ch))
    assert (got == old).all()
    fe = lambda x: oracle.from_u64(x)
    k = got.shape[0] - 1
    kids = ch[16 * k:]
    assert (got[k] == oracle.hash_with_ds_dynamic(0, 17, np.array([fe(16), fe(2), fe(k), fe(9)]), kids, kids.shape[0])).all()


@pytest.mark.parametrize("log_n", [16, 20])
def test_merkle_build_roots_equal_with_option_on_and_off(gpu_ctx, log_n):
    """stark_merkle_build_dev over 2^16 and 2^20 leaves (arity 16): the same root and the same levels with the new node kernel and without."""
    import torch
    lib = gpu_ctx.lib; p17 = gpu_ctx.poseidon_params_for_width(17)
    n = 1 << log_n
    x = torch.empty((n, 4), dtype=torch.int64, device="cuda")
    gpu_ctx._chk(lib.stark_synth_column_dev(gpu_ctx.h, 77 + log_n, 1, 0, n, C.c_void_p(x.data_ptr())))

    def build():
        t = C.c_void_p()
        gpu_ctx._chk(lib.stark_merkle_build_dev(gpu_ctx.h, p17.h, 16, 3, C.c_void_p(x.data_ptr()), n, 0, None, 0, 0, 0, C.byref(t)))
        r = np.zeros(4, np.uint64)
        gpu_ctx._chk(lib.stark_merkle_root(t, r.ctypes.data_as(C.c_void_p)))
        lib.stark_merkle_free(t)
        return r
    new = build()
    old = _with_option(gpu_ctx, b"merkle_node16_pair", 0, build)
    assert (new == old).all()
    del x; gpu_ctx.trim()


@pytest.mark.parametrize("log_n0,schedule", [(21, [16, 16, 8]), (21, [8, 16, 4]), (20, [16, 16, 8])])
def test_fri_build_roots_equal_with_side_pair_on_and_off(gpu_ctx, oracle, log_n0, schedule):
    """fri_build_transcript with the side stream's commitments in the wave-pair form (default, from 2^21 layer-0 leaves on this device) and in the
    latency forms (option "fri_side_pair" = 0), each also with the generic node kernel: the same L + 1 roots."""
    f0 = oracle.synth_column(5150 + log_n0, 0, 0, 1 << log_n0)

    def roots():
        st = gpu_ctx.fri_build_transcript(f0, schedule, 0xDEEFBAAD)
        try:
            return np.stack([st.root(l) for l in range(len(schedule) + 1)])
        finally:
            st.free()
    want = roots()
    assert (_with_option(gpu_ctx, b"fri_side_pair", 0, roots) == want).all()
    assert (_with_option(gpu_ctx, b"merkle_node16_pair", 0, roots) == want).all()
