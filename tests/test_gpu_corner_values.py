"""Stored-limb corner values through the device kernels (C-ABI) against the oracle on identical stored inputs, bit for bit.

The inputs are corners of the four u64 limbs AS STORED (tests/corner_values.py), and for the Poseidon kernels inputs crafted so that the
S-box outputs of round 0 — the words the signed radix-256 recoding in front of the int8 matrix cores reads — are chosen byte patterns
(0x80 / 0x7f carry chains across every 32-bit word, all-0xff, the band [2^254, r) ...).  The recoding, the fold and the carry pass are the host checks'
statements (mfma_digits.hpp), but the tile layout, the lane exchange and the device compilation of those statements are seen only by device runs on
chosen digits.  tests/test_corner_values_host.py checks the construction itself on the CPU.  Needs an MI355X: `pytest -m gpu`.

Chosen words in EVERY round: stark_poseidon_params_upload takes arbitrary round constants and the S-box input of every round is state + rc, so
for one chosen node the constants are picked (corner_values.steered_params / steered_node) such that all 8 t full-round S-box outputs and all rp
partial-round outputs x_q on its trajectory are chosen stored values: the recoding sees chosen digits in all eight full rounds, the carry-free
radix-2^29 accumulations of pair_permute_blk4's four-round blocks and the five-wave form's chain tables see chosen x_q at every block position, and the
uniform schedules make every term of every accumulation the same extreme at once.  Expected values under such a set come from pyref; the oracle
library knows only the fixed sets.  The wide widths t = 33 / 65 / 129 (k_hash_ds_wave and the lane form with 32-lane blocks) get the crafted
round-0 levels, and t = 33 / 65 steered sets as well; there is no steered set for t = 129, whose table derivation takes minutes.

Not steerable: tr_hash, the leaf hash and the transcripts run the context's fixed transcript set (ctx_transcript_params; stark_leaf_pair_hash_dev
rejects other constants).  They share pair_permute_blk4 / pair_permute_blk8 / pair_permute_fused / coop_permute / chain_sponge_ex with the DS kernels, which is how they are covered; their own
inputs stay at round-0 corners.  A full node's second permutation cannot be steered for GIVEN children (its input depends on every constant); it is
steered by choosing the children so that it repeats the first one's trajectory, at the price of one forced target (steered_node).

Still open: the partial-round S-box outputs are controlled now, but nothing here drives one lane of pair_lane_update to its 2.7 r bound, or the wave
form's lanes (about r per round, reduced every 32 rounds) to theirs: that would need a search over the x_q against the kernel-form w tables."""
import numpy as np
import pytest

import corner_values as cv
import pyref

pytestmark = pytest.mark.gpu

from stark_mlwe_amd.api import BLS12_381_FR, PALLAS_FR, DeepFriParams, StarkError

P = pyref.P_PALLAS
R = pyref.R
PRIMES = {PALLAS_FR: pyref.P_PALLAS, BLS12_381_FR: pyref.P_BLS}


def with_options(ctx, opts, fn):
    """run fn with context options set to `opts` ({key: (value, value to restore)}), restoring them whatever happens"""
    try:
        for k, (v, _) in opts.items():
            ctx.set_option(k, v)
        return fn()
    finally:
        for k, (_, back) in opts.items():
            ctx.set_option(k, back)


def first_diff(got, want):
    bad = np.nonzero((got != want).any(axis=1))[0]
    return None if bad.size == 0 else int(bad[0])


# ---- Poseidon: every kernel form on crafted levels ----------------------------------------------------------------------------------
# kernel forms of a Merkle level (capi_poseidon.hip poseidon_form): the default choice by size — five-wave up to 256 nodes, one-wave up to 4096,
# k_node16_pair above — and what the options force
FORMS = {"default": {}, "k_hash_ds2 (merkle_node16_pair = 0)": {"merkle_node16_pair": (0, 1)}, "lane (poseidon_lane_only = 1)": {"poseidon_lane_only": (1, 0)},
         "one-wave / wave-pair (sponge_one_wave = 1)": {"sponge_one_wave": (1, 0)}}


def check_level(ctx, oracle, dev_params, okind, params, nodes, level, pos0, label, last_children=None, forms=FORMS, uniform=False):
    t = params["t"]; arity = t - 1
    ch, slot_idx = cv.crafted_level(params, nodes, last_children=last_children, uniform=uniform)
    full = nodes if last_children is None else nodes - 1
    want = np.zeros((nodes, 4), np.uint64)
    want[:full] = oracle.hash_with_ds_dynamic(okind, t, cv.ds_words(oracle, arity, level, pos0, label, full), ch[:full * arity], arity, n=full).reshape(full, 4)
    if last_children is not None:
        want[full] = oracle.hash_with_ds_dynamic(okind, t, cv.ds_words(oracle, arity, level, pos0 + full, label, 1), ch[full * arity:], last_children)
    for name, opts in forms.items():
        got = with_options(ctx, opts, lambda: ctx.hash_ds_level(dev_params, arity, level, pos0, label, ch))
        assert got.shape == want.shape
        k = first_diff(got, want)
        assert k is None, "form %s, %d nodes, t = %d: node %d (lane %d) differs from the oracle; children (stored limbs) %s; round-0 S-box targets %s" % (
            name, nodes, t, k, k % 64, cv.hex_limbs(ch[arity * k:arity * k + arity]), cv.hex_limbs(cv.raw_array([cv.stored_corners(P)[i] for i in slot_idx[k]])))
    return slot_idx


@pytest.mark.parametrize("nodes,last", [(256, None), (257, None), (4096, None), (4097, None), (8193, None), (4100, 5)])
def test_crafted_merkle_levels_every_kernel_form(gpu_ctx, oracle, nodes, last):
    """hash_ds_level over crafted arity-16 nodes — every stored corner as the round-0 S-box output of every one of the twelve controllable
    state elements, in lanes of both 32-sponge column tiles — at the node counts on both sides of every form threshold, a ragged level, and
    under every option that changes the kernel: all forms equal the oracle's hash_with_ds_dynamic on EVERY node."""
    p17 = gpu_ctx.poseidon_params_for_width(17)
    slot_idx = check_level(gpu_ctx, oracle, p17, 0, pyref.params_for_width(17), nodes, 3, 1000, 42, last_children=last)
    if nodes > 4096:
        L = len(cv.stored_corners(P)); n_full = nodes if last is None else nodes - 1
        cover = np.zeros((L, 12, 2), bool)
        n = np.arange(n_full)
        for j in range(12):
            cover[slot_idx[:n_full, j], j, (n % 64) // 32] = True
        assert cover.all()                 # every corner in every slot in both halves of a 64-sponge block


def test_crafted_levels_other_parameter_sets_and_t9(gpu_ctx, oracle):
    """The fragment tables are derived per parameter set and t = 9 takes the L*U pair path: crafted levels (targets crafted with the set's own
    round constants) for `POSEIDON-T17-X5` and for arity 8."""
    pb = gpu_ctx.generate_params_t17_x5(b"POSEIDON-T17-X5")
    try:
        bench = pyref.derive_params(b"POSEIDON-T17-X5", 17, 8, 64)
        for nodes, last in ((257, None), (4097, None), (4099, 5)):
            check_level(gpu_ctx, oracle, pb, 3, bench, nodes, 4, 100, 42, last_children=last)
    finally:
        pb.free()
    p9 = gpu_ctx.poseidon_params_for_width(9)
    forms = {k: v for k, v in FORMS.items() if "node16" not in k}
    for nodes, last in ((300, None), (4097, None), (4098, 3)):
        check_level(gpu_ctx, oracle, p9, 0, pyref.params_for_width(9), nodes, 1, 7, 5, last_children=last, forms=forms)


@pytest.mark.parametrize("t", [9, 17, 33, 65])
def test_permute_on_corner_and_crafted_states(gpu_ctx, oracle, t):
    corners = cv.stored_corners(P); L = len(corners)
    params = base_params(t)
    rows = [[corners[(i + j) % L] for j in range(t)] for i in range(L)] + [[v] * t for v in corners]
    rows += [cv.crafted_state(params, [corners[(i + 2 * j) % L] for j in range(t)]) for i in range(L)]
    st = np.stack([cv.raw_array(r) for r in rows])
    assert st.shape[0] % 64
    got = gpu_ctx.permute(st, gpu_ctx.poseidon_params_for_width(t))
    want = oracle.permute(0, t, st)
    bad = np.nonzero((got != want).any(axis=(1, 2)))[0]
    assert bad.size == 0, "t = %d, state %d: %s" % (t, bad[0], cv.hex_limbs(st[bad[0]]))


# ---- Poseidon: the wide widths on crafted levels ---------------------------------------------------------------------------------------
_BASE = {}


def base_params(t):
    """pyref's Merkle set of width t, derived once per module (t = 129 takes seconds in Python)"""
    if t not in _BASE:
        _BASE[t] = pyref.params_for_width(t)
    return _BASE[t]


WIDE_FORMS = {"default (Wide, k_hash_ds_wave)": {}, "lane (poseidon_lane_only = 1)": {"poseidon_lane_only": (1, 0)}}


@pytest.mark.parametrize("t", [33, 65])
def test_crafted_levels_wide_widths(gpu_ctx, oracle, t):
    """k_hash_ds_wave<33 / 65> — nine lazy limbs, row eighths with a carry pass every fr29_max_terms terms — has no host twin and met only
    synth_column values so far: crafted levels (every stored corner as the round-0 S-box output of every one of the t - 5 controllable elements),
    L + 2 nodes and L + 3 with a ragged last node, rotated and uniform (one corner in every slot of a node), through the wave form and the lane form."""
    L = len(cv.stored_corners(P))
    dev = gpu_ctx.poseidon_params_for_width(t)
    for nodes, last in ((L + 2, None), (L + 3, 5)):
        for uniform in (False, True):
            slot_idx = check_level(gpu_ctx, oracle, dev, 0, base_params(t), nodes, 2, 77, 42, last_children=last, forms=WIDE_FORMS, uniform=uniform)
            full = slot_idx[:L]
            if uniform:
                assert (full == np.arange(L)[:, None]).all()
            else:
                assert all(sorted(set(full[:, j].tolist())) == list(range(L)) for j in range(t - 5))        # every corner in every slot


def test_crafted_level_t129(gpu_ctx, oracle):
    """t = 129 on the crafted level, 3 full nodes and a ragged one, under the session context's cached set (its derivation takes minutes: never a
    second one): the wave form, and the lane form, which at this width runs 32-lane blocks (poseidon_block)."""
    dev = gpu_ctx.poseidon_params_for_width(129)
    for uniform in (False, True):
        check_level(gpu_ctx, oracle, dev, 0, base_params(129), 4, 2, 77, 42, last_children=7, forms=WIDE_FORMS, uniform=uniform)


# ---- Poseidon: chosen words behind every S-box of all 72 rounds (steered round constants) ------------------------------------------------
LEVEL, LABEL = 3, 42
# lanes 0, 31, 32, 63 of the first four 64-sponge blocks: where the main sets put their steered node (all below 256, the smallest level)
INTERIOR = [0, 31, 32, 63, 64, 95, 96, 127, 128, 159, 160, 191, 192, 223, 224, 255]
# the nodes every main set is compared on besides its steered one — first, block edges, the 32-sponge tile edges, a fixed random draw.  They lie below
# 256 and a set keeps its pos0 at every level size, so their pyref digests (20 ms each at t = 17) are computed once per set, not once per call
SHARED = sorted(set([0, 1, 31, 32, 33, 62, 63, 64, 65, 127, 128, 129, 191, 192, 254, 255] + np.random.default_rng(7).choice(256, 24, replace=False).tolist()))[:32]


class SteeredSets:
    """The steered sets of one width, derived and uploaded once per module.  role "main": one per schedule (corner_values.target_schedules), first
    permutation steered, the sets the coverage is computed over; "both": both permutations of a full node steered; "edge": placed in the last
    partial block (permutation 1, and both); "ragged": the ragged last node, which has one permutation."""

    def __init__(self, ctx):
        self.ctx, self.by_t, self.memo = ctx, {}, {}

    def sets(self, t, roles=None):
        if t not in self.by_t:
            base = base_params(t); sc = cv.target_schedules(base); ragged = 5 if t == 17 else 3
            rot0 = next(i for i, s in enumerate(sc) if s[0].startswith("rotation"))
            if t <= 17:
                plan = [("main", i, 1, None) for i in range(len(sc))] + [("both", rot0, 2, None), ("both", 0, 2, None), ("edge", rot0 + 1, 1, None), ("edge", 1, 2, None), ("ragged", rot0 + 2, 1, ragged)]
            elif t == 33:
                plan = [("first", rot0, 1, None), ("last", 0, 2, None)]
            else:
                plan = [("first", rot0, 2, None)]                       # ONE set: the table derivation grows like t^4
            out = []
            for n, (role, i, which, count) in enumerate(plan):
                nd = cv.steered_set(base, sc[i], which, 5000 + 977 * n, LEVEL, LABEL, count=count)
                nd["role"] = role; nd["id"] = "t = %d, set %d (%s, %s, permutation %s steered, %d children)" % (t, n, role, nd["name"], "1" if which == 1 else "1 and 2", nd["count"])
                nd["kstar"] = INTERIOR[n % len(INTERIOR)]
                nd["dev"] = self.ctx.params_upload(*cv.params_arrays(nd["params"]))
                out.append(nd)
            self.by_t[t] = out
        return [nd for nd in self.by_t[t] if roles is None or nd["role"] in roles]

    def digest(self, nd, pos0, k, children):
        """pyref's digest of node k (not the steered one) of a level starting at pos0 under the set nd, memoised: the children of a crafted level
        depend on the index alone"""
        key = (nd["id"], pos0, k, children.shape[0])
        if key not in self.memo:
            self.memo[key] = cv.node_digest(nd["params"], LEVEL, pos0 + k, LABEL, children)
        return self.memo[key]

    def free(self):
        for sets in self.by_t.values():
            for nd in sets:
                nd["dev"].free()
        self.by_t = {}


@pytest.fixture(scope="module")
def steered(gpu_ctx):
    s = SteeredSets(gpu_ctx)
    yield s
    s.free()


def check_steered_level(ctx, steered, nd, nodes, kstar, last, forms, sample):
    """hash_ds_level under the steered set nd over a crafted level with the steered node at index kstar: the steered node against the digest the
    construction predicts, the nodes of `sample` against pyref under the same set, in every form."""
    t = nd["t"]; arity = t - 1
    ch, pos0 = cv.steered_level(base_params(t), nd, nodes, kstar, last_children=last)
    sample = set(k for k in sample if 0 <= k < nodes and k != kstar)
    for k in range(2, nodes, 7):                                              # top up to 32 others (the same ones at every level size)
        if len(sample) >= 32:
            break
        if k != kstar:
            sample.add(k)
    sample = sorted(sample)
    assert len(sample) >= 32
    want = {k: steered.digest(nd, pos0, k, ch[k * arity:(k + 1) * arity]) for k in sample}
    want[kstar] = nd["digest"]
    for name, opts in forms.items():
        got = with_options(ctx, opts, lambda: ctx.hash_ds_level(nd["dev"], arity, LEVEL, pos0, LABEL, ch))
        assert got.shape == (nodes, 4)
        for k in [kstar] + sample:
            assert (got[k] == want[k]).all(), "form %s, %d nodes, %s, steered node %d (lane %d, DS position %d): node %d (lane %d)%s differs from pyref under the same set: got %s want %s; " \
                "full-round targets %s; partial-round targets %s" % (name, nodes, nd["id"], kstar, kstar % 64, nd["pos"], k, k % 64, " — the steered one" if k == kstar else "",
                                                                       cv.hex_limbs(got[k]), cv.hex_limbs(want[k]), [cv.hex_limbs(cv.raw_array(r)) for r in nd["tf"]] if k == kstar else "-",
                                                                       cv.hex_limbs(cv.raw_array(nd["tp"])) if k == kstar else "-")


def test_steered_sets_cover_every_round_half_and_block_position(steered):
    """Coverage by computation, over the values the S-boxes of the main sets really deliver (recomputed from the uploaded constants' trajectory, not
    read off the schedule): every stored corner in every one of the 8 full rounds — for t = 17 in both element halves X and Y of the wave pair
    (PairCfg::NX) — and as x_q at every block position q mod 4; each uniform schedule present.  The number of sets is what the windows need:
    9 uniform schedules and ceil(37 / 8) = 5 rotations for t = 17 (the X half has 8 elements), ceil(37 / 9) = 5 for t = 9.
    Deriving the tables of an uploaded set is host work that grows like t^4: measured on a slow development CPU 0.08 s at t = 9, 0.37 s at
    t = 17, 2.3 s at t = 33 and 18 s at t = 65; on the MI355X host this whole test, 38 uploads, takes 1.1 s.  Hence no set more than needed."""
    corners = cv.stored_corners(P)
    for t in (17, 9):
        main = steered.sets(t, ("main",))
        assert len(main) == 14
        got = []
        for nd in main:
            of, op, _ = cv.sbox_outputs(nd["params"], nd["state"])
            assert of == nd["tf"] and op == nd["tp"], nd["id"]
            got.append((of, op))
        full, part, uni = cv.schedule_coverage(t, got)
        assert full.shape == (len(corners), 8, 2 if t == 17 else 1)
        assert full.all(), "t = %d: corner / full round / half never met: %s" % (t, np.argwhere(~full)[:5].tolist())
        assert part.all(), "t = %d: corner / q mod 4 never met: %s" % (t, np.argwhere(~part)[:5].tolist())
        assert uni >= {P - 1, (1 << 254) - 1, 1 << 254, cv.alt29(0), cv.alt29(1)} | set(cv.carry_chains())
        for nd in steered.sets(t, ("both",)):                                 # the second permutation starts from the first one's input state
            of, op, end = cv.sbox_outputs(nd["params"], nd["state"])
            assert of == nd["tf"] and op == nd["tp"], nd["id"]
            kids = [cv.raw_to_int(x) * pow(R, -1, P) % P for x in nd["children"]]
            absorb = kids[t - 5:] + [1] + [0] * (t - 5)
            assert [(end[i] + absorb[i]) % P for i in range(t)] == nd["state"] and end[0] * R % P == cv.raw_to_int(nd["digest"]), nd["id"]


# (t, nodes, children of a ragged last node): the node counts that select each form — five-wave up to 256, one-wave up to 4096, k_node16_pair above
# (k_hash_ds2 with merkle_node16_pair = 0, and for a ragged level) — and for t = 9, which has no node16 form, both sides of 4096 and a ragged level
STEERED_LEVELS = [(17, 256, None), (17, 257, None), (17, 4097, None), (17, 4100, 5), (9, 300, None), (9, 4097, None), (9, 4098, 3)]


@pytest.mark.parametrize("t,nodes,last", STEERED_LEVELS)
def test_steered_nodes_every_merkle_level_form(gpu_ctx, steered, t, nodes, last):
    """A node whose S-box outputs are chosen stored corners in ALL rounds — 8 t full-round outputs and rp partial-round outputs x_q — through every
    form of a Merkle level, at the node counts that select the forms and under every option that changes the kernel.  Main sets and the sets with
    both permutations steered sit at lanes 0 / 31 / 32 / 63 of a 64-sponge block; the edge sets in the last partial block; one set is the ragged
    last node (one permutation).  The steered node must equal the digest the construction predicts, and >= 32 other nodes (crafted_level children)
    per call pyref's hash_with_ds_dynamic under the same uploaded set.
    Measured on the MI355X host: 3.7 s for the first t = 17 case (it computes the pyref digests the later ones share), 0.5 to 1.8 s for the others;
    pyref, not the device, is the time of this test."""
    forms = FORMS if t == 17 else {k: v for k, v in FORMS.items() if "node16" not in k}
    rng = np.random.default_rng(nodes)
    tail = [nodes - 1, nodes - 2, (nodes - 1) // 64 * 64, (nodes - 1) // 64 * 64 - 1, (nodes - 1) // 32 * 32 - 1] + rng.integers(0, nodes, 4).tolist()
    for nd in steered.sets(t, ("main", "both")):
        check_steered_level(gpu_ctx, steered, nd, nodes, nd["kstar"], last, forms, SHARED + tail)
    n_full = nodes if last is None else nodes - 1
    if n_full % 64:                                                           # a last partial block: its full nodes, first permutation and both
        for j, nd in enumerate(steered.sets(t, ("edge",))):
            kstar = n_full - 1 - j if n_full % 64 > j else n_full - 1
            check_steered_level(gpu_ctx, steered, nd, nodes, kstar, last, forms, SHARED[:24] + tail + rng.integers(0, nodes, 6).tolist())
    if last is not None:
        for nd in steered.sets(t, ("ragged",)):
            check_steered_level(gpu_ctx, steered, nd, nodes, nodes - 1, last, forms, SHARED[:24] + tail + rng.integers(0, nodes, 6).tolist())


@pytest.mark.parametrize("t", [33, 65])
def test_steered_nodes_wide_widths(gpu_ctx, steered, t):
    """Steered nodes through k_hash_ds_wave and the lane form at t = 33 and t = 65, at index 0 and at the last index of a level of 34 nodes, 33
    others per call against pyref.  t = 33: one set with the first permutation steered, one with both.  t = 65: ONE set, both permutations
    steered: the derivation of an uploaded set's tables grows like t^4 and a pyref permutation takes 0.13 s at this width.  Measured on the
    MI355X host: 1.9 s (t = 33) and 7.0 s (t = 65), nearly all of it on the CPU.  No t = 129 set: its derivation takes far longer."""
    nodes = 34
    sets = steered.sets(t)
    for nd, kstar in ((sets[0], 0), (sets[-1], nodes - 1)):
        check_steered_level(gpu_ctx, steered, nd, nodes, kstar, None, WIDE_FORMS, range(nodes))


@pytest.mark.parametrize("t", [9, 17, 33, 65])
def test_permute_on_steered_states(gpu_ctx, steered, t):
    """k_permute_batch under every steered set of the width: 65 copies of the steered state (more than one 64-lane block) and 5 other states,
    against the end state the construction predicts and pyref under the same set."""
    rng = np.random.default_rng(t)
    others = [[int.from_bytes(rng.bytes(40), "little") % P for _ in range(t)] for _ in range(3)] + [[0] * t, [P - 1] * t]
    for nd in steered.sets(t):
        if nd["role"] not in ("main", "first", "last", "both"):
            continue
        sp = nd["params"]
        end = cv.sbox_outputs(sp, nd["state"])[2]
        st = np.stack([cv.to_stored(nd["state"])] * 65 + [cv.to_stored(s) for s in others])
        want = np.stack([cv.to_stored(end)] * 65 + [cv.to_stored(pyref.permute(s, sp)) for s in others])
        got = gpu_ctx.permute(st, nd["dev"])
        bad = np.nonzero((got != want).any(axis=(1, 2)))[0]
        assert bad.size == 0, "k_permute_batch, %s: state %d (0..64 are the steered one) differs from pyref: got %s want %s" % (nd["id"], bad[0], cv.hex_limbs(got[bad[0]])[:2], cv.hex_limbs(want[bad[0]])[:2])


@pytest.mark.parametrize("n", [2048, 2049, 4096, 4097, 1 << 13])
def test_leaf_pair_hash_on_corners(gpu_ctx, oracle, n):
    corners = cv.raw_array(cv.stored_corners(P)); L = corners.shape[0]
    rng = np.random.default_rng(n)
    f = corners[rng.integers(0, L, n)]; fn = corners[rng.integers(0, L, (n + 15) // 16)]
    f[:L] = corners; f[n - L:] = corners[::-1]; fn[:L] = corners
    for m, nxt in ((16, fn), (1, None)):
        got, want = gpu_ctx.leaf_pair_hash(f, nxt, m), oracle.leaf_pair_hash(f, nxt, m)
        k = first_diff(got, want)
        assert k is None, "m = %d, %d leaves: leaf %d f = %s" % (m, n, k, cv.hex_limbs(f[k]))
    got = with_options(gpu_ctx, {"poseidon_lane_only": (1, 0)}, lambda: gpu_ctx.leaf_pair_hash(f, fn, 16))
    assert (got == oracle.leaf_pair_hash(f, fn, 16)).all()


@pytest.mark.parametrize("n", [512, 513, 4097])
def test_tr_hash_on_corners(gpu_ctx, oracle, n):
    x = cv.pattern_d(P, 3 * n)
    got = gpu_ctx.tr_hash_fields_tagged(b"FRI/index", x, n=n)
    for i in range(n):
        assert (got[i] == oracle.tr_hash_fields_tagged(b"FRI/index", x[3 * i:3 * i + 3])).all(), (n, i, cv.hex_limbs(x[3 * i:3 * i + 3]))


def test_merkle_tree_over_crafted_leaves(gpu_ctx, oracle):
    """arity-16 merkle_new over 2^17 leaves that are the children of 8192 crafted nodes: every level against the oracle's tree."""
    leaves, _ = cv.crafted_level(pyref.params_for_width(17), 1 << 13)
    assert leaves.shape[0] == 1 << 17
    t = gpu_ctx.merkle_new(leaves, gpu_ctx.merkle_cfg(16, 3)); o = oracle.merkle_build(16, 3, leaves)
    try:
        assert t.num_levels == o.num_levels()
        for lvl in range(o.num_levels()):
            assert (t.level(lvl) == o.level(lvl)).all(), lvl
    finally:
        t.free(); o.free()


# ---- NTT ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field,gen", [(PALLAS_FR, 5), (BLS12_381_FR, 7)])
@pytest.mark.parametrize("lg", [3, 10, 12, 13, 16, 20, 21])
def test_ntt_on_stored_extremes(gpu_ctx, oracle, field, gen, lg):
    """fft / ifft / coset fft / lde on whole vectors of stored p - 1, stored 2^254 - 1, two alternating patterns and the corner list by index."""
    p = PRIMES[field]; n = 1 << lg
    g = oracle.from_u64(gen, field)
    for name, x in cv.patterns(p, n).items():
        assert (gpu_ctx.fft(x, field=field) == oracle.ntt(field, x)).all(), (field, lg, name, "fft")
        assert (gpu_ctx.ifft(x, field=field) == oracle.ntt(field, x, inverse=True)).all(), (field, lg, name, "ifft")
        assert (gpu_ctx.fft(x, field=field, coset=g) == oracle.ntt(field, x, coset=g)).all(), (field, lg, name, "coset fft")
        assert (gpu_ctx.ifft(x, field=field, coset=g) == oracle.ntt(field, x, inverse=True, coset=g)).all(), (field, lg, name, "coset ifft")
        if lg < 4:
            continue
        ev = x[:n >> 3]
        assert (gpu_ctx.lde(ev, 3, field=field, coset=g) == oracle.lde(field, ev, 3, g)).all(), (field, lg, name, "lde")


def test_ntt_two_level_twiddles_and_tiles_on_stored_extremes(oracle):
    """The two-level twiddle lookup (ntt_direct_max_log = 0) and the 2^9 / 2^12 tiles on a second context, at 2^21, on the corner list by index
    and on all-(p - 1), against the oracle."""
    from stark_mlwe_amd.api import Context
    g = oracle.from_u64(5)
    pats = cv.patterns(P, 1 << 21)
    c = Context(0)
    try:
        c.set_option("ntt_direct_max_log", 0)
        for name in ("corners by index", "all p-1"):
            x = pats[name]; y = oracle.ntt(0, x); z = oracle.ntt(0, x, coset=g)
            assert (c.fft(x, field=PALLAS_FR) == y).all() and (c.fft(x, field=PALLAS_FR, coset=g) == z).all(), name
            assert (c.ifft(z, field=PALLAS_FR, coset=g) == x).all(), name
            for tile in (9, 12, -1):
                c.set_option("ntt_log_tile", tile)
                assert (c.fft(x, field=PALLAS_FR, coset=g) == z).all(), (name, tile)
    finally:
        c.close()


@pytest.mark.parametrize("log_n,log_rows", [(16, 8), (20, 10)])
def test_six_step_building_blocks_on_stored_extremes(gpu_ctx, oracle, log_n, log_rows):
    import torch
    from stark_mlwe_amd import dist as sd
    n = 1 << log_n
    pats = cv.patterns(P, n)
    plan = sd.DistNtt(sd.HipProvider(gpu_ctx), log_n, log_rows, inverse=False)
    for name in ("corners by index", "all p-1", "alternating 29-bit limb phases"):
        x = pats[name]
        slab = torch.from_numpy(x[plan.local_input_indices().reshape(-1).numpy()].view(np.int64).copy()).cuda()
        rows = plan.forward(slab, None)
        gpu_ctx.sync()
        nat = plan.to_natural_blocks(rows).cpu().numpy().view(np.uint64)
        assert (nat == oracle.ntt(0, x)).all(), name


# ---- FRI fold / ALI merge ---------------------------------------------------------------------------------------------------------------
Z_STORED = [P - 1, (1 << 254) - 1, 1 << 254, R % P]


@pytest.mark.parametrize("m", [2, 4, 8, 16, 32, 64, 128, 3, 6])
def test_fri_fold_on_corners(gpu_ctx, oracle, m):
    n = m * 37 if m in (3, 6) else max(m * 5, 1 << 11)
    f = cv.pattern_d(P, n)
    for zs in Z_STORED:
        z = cv.raw(zs)
        assert (gpu_ctx.fri_fold_layer(f, z, m) == oracle.fri_fold_layer(f, z, m)).all(), (m, hex(zs))
        assert (gpu_ctx.compute_s_layer(f, z, m) == oracle.compute_s_layer(f, z, m)).all(), (m, hex(zs))


@pytest.mark.parametrize("n", [64, 1000, 1 << 12])
def test_ali_merge_on_corners(gpu_ctx, oracle, n):
    c = cv.pattern_d(P, n + 4 * 7)
    cols = [c[7 * k:7 * k + n] for k in range(5)]                      # the corner list by index, each column at its own offset
    lg = (n - 1).bit_length()
    omega, beta = oracle.root_of_unity(lg), cv.raw((1 << 254) + 1)
    for zs in Z_STORED:
        z = cv.raw(zs)
        if pow(zs * pow(R, -1, P) % P, 1 << lg, P) == 1:               # z in the domain (stored R mod p is the logical 1)
            with pytest.raises(StarkError):
                gpu_ctx.deep_ali_merge_evals(cols[0], cols[1], cols[2], cols[3], omega, z)
            continue
        f0, _, cs = gpu_ctx.deep_ali_merge_evals(cols[0], cols[1], cols[2], cols[3], omega, z)
        w0, wc = oracle.ali_merge(cols[0], cols[1], cols[2], cols[3], omega, z)
        assert (f0 == w0).all(), (n, hex(zs))
        if n == 1 << lg:
            assert (cs == wc).all(), (n, hex(zs))
        f1, _, _ = gpu_ctx.deep_ali_merge_evals(cols[0], cols[1], cols[2], cols[3], omega, z, r_eval=cols[4], beta=beta, want_c_star=False)
        w1, _ = oracle.ali_merge(cols[0], cols[1], cols[2], cols[3], omega, z, r=cols[4], beta=beta, want_c_star=False)
        assert (f1 == w1).all(), (n, hex(zs))
    assert any(pow(zs * pow(R, -1, P) % P, 1 << lg, P) == 1 for zs in Z_STORED)


def test_fri_transcript_and_prove_on_corners(gpu_ctx, oracle):
    n0, sched, r, seed_z = 1 << 11, [16, 16, 8], 32, 0xDEEFBAAD
    c = cv.pattern_d(P, n0 + 33)
    f0 = c[:n0]
    st = gpu_ctx.fri_build_transcript(f0, sched, seed_z)
    ref = oracle.deep_fri_prove(None, None, None, None, n0, sched, 1, seed_z, f0=f0)
    try:
        for l in range(st.num_layers):
            assert (st.f_layer(l) == ref.layer_f(l)).all() and (st.root(l) == ref.root(l)).all(), l
            if l < len(sched):
                assert (st.z(l) == ref.z(l)).all()
    finally:
        st.free(); ref.free()
    cols = [c[11 * k:11 * k + n0] for k in range(4)]
    got, est, _ = gpu_ctx.deep_fri_prove(cols[0], cols[1], cols[2], cols[3], n0, DeepFriParams(sched, r, seed_z))
    ref = oracle.deep_fri_prove(cols[0], cols[1], cols[2], cols[3], n0, sched, r, seed_z)
    try:
        assert got == ref.bytes() and est == ref.size_estimate()
        assert oracle.deep_fri_verify(got, sched, r, seed_z) == 1
    finally:
        ref.free()


# ---- sum-check ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 4, 12])
def test_sumcheck_on_corners(gpu_ctx, oracle, k):
    import torch
    pats = cv.patterns(P, 1 << k)
    ws = [pats["corners by index"], pats["all p-1"], pats["alternating 29-bit limb phases"]]
    labels = [2025, 7, 5050]; q = 2
    want = [[oracle.sumcheck_prove(mf, k, labels[b], ws[b], q=q) for b in range(3)] for mf in (0, 1)]
    for mf in (0, 1):
        for b in range(3):
            assert oracle.sumcheck_verify(mf, k, labels[b], want[mf][b], q=q) == 1
    for b in range(2):
        assert gpu_ctx.prove_plain(k, labels[b], ws[b]) == want[0][b], b
        assert gpu_ctx.prove_mf(k, labels[b], q, ws[b]) == want[1][b], b
    ts = [torch.from_numpy(np.ascontiguousarray(w).view(np.int64)).to("cuda") for w in ws]
    torch.cuda.synchronize()
    ptrs = [t.data_ptr() for t in ts]
    for B in (1, 3):
        assert gpu_ctx.prove_plain_batch_dev(k, labels[:B], ptrs[:B]) == want[0][:B], B
        assert gpu_ctx.prove_mf_batch_dev(k, labels[:B], q, ptrs[:B]) == want[1][:B], B
    assert gpu_ctx.verify_plain(k, labels[0], want[0][0]) is True and gpu_ctx.verify_mf(k, labels[0], q, want[1][0]) is True
