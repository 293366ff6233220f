"""Input families for the stored-limb corner tests (test infrastructure, plain Python + numpy).

Field elements cross every boundary of this project as four u64 limbs in Montgomery form, and the delicate kernel arithmetic (lazy nine-limb
butterflies, fr29_partial_reduce, the wide dots' carry passes, the signed radix-256 recoding in front of the int8 matrix cores) is sensitive
to those STORED limbs.  A corner of the logical value passed through `from_int` reaches the code as ordinary random-looking words; the values
here are corners of the stored limbs themselves, and `sbox_preimage` / `crafted_children` / `crafted_state` place chosen stored words behind
the first S-box, where the recoding reads them."""
import math

import numpy as np

import pyref

R = pyref.R
M64 = (1 << 64) - 1
M29 = (1 << 29) - 1
SBOX_SHIFT = 20          # fr29.hpp FR29_SBOX_SHIFT: the kernels' S-box fr_pow5_r29 delivers the stored limbs of x^5 divided by 2^20


def raw(v):
    """integer -> four u64 limbs AS STORED (no Montgomery conversion)"""
    assert 0 <= v < 1 << 256
    return np.array([(v >> (64 * i)) & M64 for i in range(4)], np.uint64)


def raw_to_int(a):
    a = np.asarray(a, np.uint64).reshape(4)
    return sum(int(a[i]) << (64 * i) for i in range(4))


def raw_array(vals):
    """list of integers -> (n, 4) uint64 array of stored limbs"""
    return np.stack([raw(v) for v in vals]) if len(vals) else np.zeros((0, 4), np.uint64)


def hex_limbs(a):
    """stored limbs of one element or of an array of elements, as hex strings (for assertion messages)"""
    a = np.asarray(a, np.uint64).reshape(-1, 4)
    return ["%064x" % raw_to_int(x) for x in a]


def _from_bytes_le(bs):
    assert len(bs) == 32
    return int.from_bytes(bytes(bs), "little")


def carry_chains():
    """0x80 followed by 0x7f bytes up to byte 30 (top byte 0): adding 0x80 to every byte carries out of the first byte and through every later
    one — the longest carry chain of recode_signed, across all seven 32-bit word boundaries — and the same chain started at byte offsets 3, 4, 7."""
    return [_from_bytes_le([0] * off + [0x80] + [0x7f] * (30 - off) + [0]) for off in (0, 3, 4, 7)]


def alt29(phase):
    """maximal 29-bit limbs at the even (phase 0) or odd (phase 1) limb positions, zero between them, clipped to 254 bits"""
    return sum(M29 << (29 * i) for i in range(9) if i % 2 == phase) & ((1 << 254) - 1)


def alt32(phase):
    """0xffffffff at the even (phase 0) or odd (phase 1) 32-bit words, zero between them, clipped to 254 bits"""
    return sum(0xffffffff << (32 * i) for i in range(8) if i % 2 == phase) & ((1 << 254) - 1)


def stored_corners(p):
    """Stored values (integers below p, to be passed through `raw`), without duplicates, in a fixed order."""
    top = (p >> 248) - 1                                     # the largest top byte that keeps any lower bytes below p
    vals = [0, 1, 2, p - 1, p - 2, (1 << 254) - 1, 1 << 254, (1 << 254) + 1, R % p, p - R % p, (p - 1) // 2]
    vals += [_from_bytes_le([b] * 31 + [min(b, top)]) for b in (0x7f, 0x80, 0x81, 0xfe, 0xff, 0x01)]
    vals += carry_chains()
    vals += [alt29(0), alt29(1), alt32(0), alt32(1)]
    for k in (28, 29, 31, 32, 57, 58, 63, 64, 231, 232, 253):
        vals += [1 << k, (1 << k) - 1]
    out = []
    for v in vals:
        assert 0 <= v < p, hex(v)
        if v not in out:
            out.append(v)
    return out


def pattern_d(p, n):
    """i -> stored_corners(p)[i mod len] as an (n, 4) array"""
    c = raw_array(stored_corners(p))
    return c[np.arange(n) % c.shape[0]]


def patterns(p, n):
    """the named whole-vector patterns of the NTT / fold / sum-check tests: {name: (n, 4) stored array}"""
    i = np.arange(n)
    two = lambda a, b: raw_array([a, b])[i & 1]
    return {"all p-1": np.tile(raw(p - 1), (n, 1)), "all 2^254-1": np.tile(raw((1 << 254) - 1), (n, 1)),
            "alternating p-1 / 0": two(p - 1, 0), "alternating 29-bit limb phases": two(alt29(0), alt29(1)), "corners by index": pattern_d(p, n)}


# ---- chosen stored words behind the first S-box -----------------------------------------------------------------------------------
def stored_rc(params, r, i, p=pyref.P_PALLAS):
    """round constant i of full round r of a pyref parameter set (canonical integers), as the kernels hold it"""
    return params["rc_full"][r][i] * R % p


def sbox_preimage(stored_target, rc_stored, p=pyref.P_PALLAS, shift=SBOX_SHIFT):
    """the stored x for which the kernels' S-box fr_pow5_r29(x + rc) has exactly `stored_target` as its stored limbs — the limbs the signed
    radix-256 recoding reads.  fr_pow5_r29 takes three Montgomery steps by 2^261 on operands carrying R = 2^256, so it returns the stored limbs
    of x^5 divided by 2^20 (the matrices carry the 2^20); shift = 0 gives the preimage under a plain Montgomery x^5."""
    assert math.gcd(5, p - 1) == 1
    y = (stored_target << shift) * pow(R, -1, p) % p         # logical S-box output
    u = pow(y, pow(5, -1, p - 1), p)                         # logical S-box input
    return (u * R - rc_stored) % p


def crafted_state(params, targets, p=pyref.P_PALLAS):
    """a whole state (t stored integers) whose round-0 S-box outputs are the t given stored targets"""
    assert len(targets) == params["t"]
    return [sbox_preimage(tg, stored_rc(params, 0, i, p), p) for i, tg in enumerate(targets)]


def crafted_children(params, targets, p=pyref.P_PALLAS, tail=None):
    """The t - 1 children (stored integers) of a full node of hash_with_ds_dynamic such that in round 0 of the first permutation the S-box
    outputs of state elements 4..t-2 (children 0..t-6: elements 0..3 are the DS words, t-1 the capacity) are the given stored targets.  The last
    four children, absorbed after the first permutation, are `tail` (default: the first stored corners)."""
    t = params["t"]
    assert len(targets) == t - 5
    tail = stored_corners(p)[:4] if tail is None else list(tail)
    assert len(tail) == 4
    return [sbox_preimage(tg, stored_rc(params, 0, 4 + j, p), p) for j, tg in enumerate(targets)] + tail


def crafted_level(params, nodes, p=pyref.P_PALLAS, corners=None, last_children=None, uniform=False):
    """A Merkle level of `nodes` crafted nodes of arity t - 1: node n takes the corner list rotated by n — target of slot j = corners[(n + j) % L],
    tail children from the following positions — so that over any L consecutive nodes every corner meets every controllable slot; with `uniform`
    every slot of node n has the target corners[n % L] (all terms of round 0's sums extreme at once).  `last_children` truncates the last node (a
    ragged level).  Returns ((n_children, 4) stored array, (nodes, t - 5) array of corner indices per slot)."""
    t = params["t"]; ns = t - 5
    corners = stored_corners(p) if corners is None else corners
    L = len(corners)
    pre = raw_array([sbox_preimage(c, stored_rc(params, 0, 4 + j, p), p) for j in range(ns) for c in corners]).reshape(ns, L, 4)
    cr = raw_array(corners)
    n = np.arange(nodes)[:, None]
    slot_idx = (n + (0 if uniform else 1) * np.arange(ns)[None, :]) % L
    tail_idx = (n + ns + np.arange(4)[None, :]) % L
    ch = np.concatenate([pre[np.arange(ns)[None, :], slot_idx], cr[tail_idx]], axis=1)        # (nodes, t - 1, 4)
    ch = np.ascontiguousarray(ch.reshape(-1, 4))
    if last_children is not None:
        ch = ch[:(nodes - 1) * (t - 1) + last_children].copy()
    return ch, slot_idx


def ds_words(oracle, arity, level, pos0, label, nodes):
    """the four DS words [arity, level, pos0 + k, label] of every node of a level, as an (nodes * 4, 4) array"""
    a, l, lb = oracle.from_u64(arity), oracle.from_u64(level), oracle.from_u64(label)
    return np.stack([x for k in range(nodes) for x in (a, l, oracle.from_u64(pos0 + k), lb)])


def mds_pre_canonical(params, p=pyref.P_PALLAS):
    """B_1 * M of the sparse partial-round factorisation (M_R = M, M_{k-1} = diag(1, Mhat_k) * M with Mhat_k = M_k[1:, 1:]), canonical integers"""
    t, M = params["t"], params["mds"]
    cur = [row[:] for row in M]
    for _ in range(params["rp"]):
        nxt = [M[0][:]]
        for i in range(1, t):
            nxt.append([sum(cur[i][q] * M[q][j] for q in range(1, t)) % p for j in range(t)])
        cur = nxt
    return cur


# ---- chosen stored words behind EVERY S-box: steered round constants ------------------------------------------------------------------
# The S-box input of every round is state + rc, and stark_poseidon_params_upload takes arbitrary round constants (make_kernel_consts keeps
# rc_partial as given; the MDS, and with it the kernel-form factorisation, is untouched).  So for ONE input state the constants can be chosen so
# that every S-box output on that state's trajectory — 8 t full-round outputs and rp partial-round outputs x_q — is a chosen stored value.
# Once round 0 delivers its targets the state of every later round is M times the targets before it: only the round-0 constants depend on the
# input state.  All values here are canonical integers as in pyref unless a name says `stored`.
_ROOTS = {}


def target_logical(stored_target, p=pyref.P_PALLAS):
    """the logical S-box output whose limbs, as fr_pow5_r29 delivers them (x^5 / 2^20 in the stored domain), are `stored_target`"""
    return (stored_target << SBOX_SHIFT) * pow(R, -1, p) % p


def restored(y, p=pyref.P_PALLAS):
    """the stored limbs fr_pow5_r29 delivers for the logical S-box output y (inverse of target_logical)"""
    return y * R * pow(1 << SBOX_SHIFT, -1, p) % p


def fifth_root(y, p=pyref.P_PALLAS):
    if (y, p) not in _ROOTS:
        _ROOTS[(y, p)] = pow(y, pow(5, -1, p - 1), p)
    return _ROOTS[(y, p)]


def _mds(params, s, p):
    t = params["t"]
    return [sum(params["mds"][i][j] * s[j] for j in range(t)) % p for i in range(t)]


def steered_params(params, state, targets_full, targets_partial, p=pyref.P_PALLAS):
    """(params', end_state): params with its round constants replaced so that pyref.permute(state, params') puts targets_full[r][i] (stored
    integers below p, r over the rf full rounds) and targets_partial[q] behind the S-boxes, and the state that permutation ends in."""
    t, rf, rp = params["t"], params["rf"], params["rp"]
    assert len(state) == t and len(targets_full) == rf and all(len(r) == t for r in targets_full) and len(targets_partial) == rp
    s = list(state); rcf, rcp = [], []

    def full(r):
        nonlocal s
        y = [target_logical(tg, p) for tg in targets_full[r]]
        rcf.append([(fifth_root(y[i], p) - s[i]) % p for i in range(t)])
        s = _mds(params, y, p)
    for r in range(rf // 2):
        full(r)
    for q in range(rp):
        y = target_logical(targets_partial[q], p)
        rcp.append((fifth_root(y, p) - s[0]) % p)
        s[0] = y; s = _mds(params, s, p)
    for r in range(rf // 2, rf):
        full(r)
    return dict(params, rc_full=rcf, rc_partial=rcp), s


def sbox_outputs(params, state, p=pyref.P_PALLAS):
    """the permutation of pyref.permute, recording what each S-box delivers as STORED values (`restored`): (full [rf][t], partial [rp], end state)"""
    t, half = params["t"], params["rf"] // 2
    s = list(state); of, op = [], []
    for r in range(params["rf"]):
        if r == half:
            for q in range(params["rp"]):
                s[0] = pow((s[0] + params["rc_partial"][q]) % p, 5, p); op.append(restored(s[0], p)); s = _mds(params, s, p)
        s = [pow((s[i] + params["rc_full"][r][i]) % p, 5, p) for i in range(t)]; of.append([restored(y, p) for y in s]); s = _mds(params, s, p)
    return of, op, s


def first_state(params, ds, children):
    """the state hash_with_ds_dynamic permutes first: the four DS words, the first t - 5 children (a shorter list is followed by the closing 1)"""
    t = params["t"]
    stream = list(ds) + list(children) + [1]
    return (stream + [0] * t)[:t - 1] + [0]


def steered_node(params, ds, children, which, targets_full, targets_partial, p=pyref.P_PALLAS):
    """Steered constants for one node of hash_with_ds_dynamic(ds, children): (params', children', digest, targets_full').

    which = 1: the first permutation follows the targets; the children are used as given.  A node whose stream (4 DS words, the children, the
    closing 1) fits one block of t - 1 has no other permutation; a full node's second permutation runs the same constants from whatever state the
    first one left, and the digest comes from pyref.
    which = 2 (full nodes, t - 1 children): the SECOND permutation follows the targets.  Its input is the first one's output plus the last four
    children and the closing 1, and the first one's output depends on all constants, so the second cannot be steered for given children.  But
    a steered permutation ends in M * (last round's targets) whatever its input was.  So the children are chosen here instead (`children` gives
    their number only) such that the second input state EQUALS the first: both permutations then follow the same trajectory.  That needs
    (M y)[t - 1] = 0 for the last round's logical outputs y — the capacity element absorbs nothing — which fixes ONE target, last round, element
    t - 1; targets_full' holds the value it takes."""
    t = params["t"]; rate = t - 1
    tf = [list(r) for r in targets_full]
    if which == 1:
        sp, end = steered_params(params, first_state(params, ds, children), tf, targets_partial, p)
        if 4 + len(children) + 1 <= rate:
            return sp, list(children), end[0], tf
        return sp, list(children), pyref.hash_with_ds_dynamic(ds, children, sp, p), tf
    assert which == 2 and len(children) == rate and len(ds) == 4
    M = params["mds"]
    y = [target_logical(tg, p) for tg in tf[-1]]
    y[t - 1] = -sum(M[t - 1][j] * y[j] for j in range(t - 1)) * pow(M[t - 1][t - 1], -1, p) % p
    tf[-1][t - 1] = restored(y[t - 1], p)
    o = _mds(params, y, p)                                            # where both permutations end
    assert o[t - 1] == 0
    kids = [(o[4] + 1) % p] + o[5:t - 1] + [(ds[i] - o[i]) % p for i in range(4)]
    sp, end = steered_params(params, first_state(params, ds, kids), tf, targets_partial, p)
    assert end == o
    return sp, kids, o[0], tf


def to_stored(vals, p=pyref.P_PALLAS):
    """canonical integers -> (n, 4) array of stored (Montgomery) limbs"""
    return raw_array([v * R % p for v in vals])


def params_arrays(params, p=pyref.P_PALLAS):
    """(t, rf, rp, mds, rc_full, rc_partial) of a pyref parameter set as the upload entry points take them: stored limbs, row-major"""
    t = params["t"]
    return (t, params["rf"], params["rp"], to_stored([params["mds"][i][j] for i in range(t) for j in range(t)], p),
            to_stored([x for r in params["rc_full"] for x in r], p), to_stored(params["rc_partial"], p))


def uniform_corners(p=pyref.P_PALLAS):
    """the corners that get a schedule of their own with ONE value in every slot of every round: all terms of every accumulation maximal at once"""
    return [p - 1, (1 << 254) - 1, 1 << 254, alt29(0), alt29(1)] + carry_chains()


def element_halves(t):
    """the element ranges a rotation must cover separately: the wave pair's X and Y halves for t = 17 (poseidon_pair.hpp PairCfg::NX)"""
    return [(0, 8), (8, 17)] if t == 17 else [(0, t)]


def target_schedules(params, p=pyref.P_PALLAS):
    """[(name, targets_full [rf][t], targets_partial [rp])] over stored_corners(p): the uniform schedules, then the fewest rotations of the other
    corners such that every one of them is the S-box output of every full round in every element half, and x_q at every position q mod 4 of the
    four-round partial blocks.  Rotation k gives half (a, b) the window [k (b - a), (k + 1)(b - a)) of the list, shifted by r in round r, and gives
    block position q mod 4 the window [k rp/4, (k + 1) rp/4) shifted by 5 (q mod 4): the windows of the sets tile the list."""
    t, rf, rp = params["t"], params["rf"], params["rp"]
    uni = uniform_corners(p)
    rest = [c for c in stored_corners(p) if c not in uni]; n = len(rest)
    out = [("uniform %064x" % c, [[c] * t for _ in range(rf)], [c] * rp) for c in uni]
    halves = element_halves(t); nb = rp // 4
    sets = max(-(-n // min(b - a for a, b in halves)), -(-n // nb))
    for k in range(sets):
        tf = [[0] * t for _ in range(rf)]
        for r in range(rf):
            for a, b in halves:
                for i in range(a, b):
                    tf[r][i] = rest[(k * (b - a) + (i - a) + r) % n]
        tp = [rest[(k * nb + q // 4 + 5 * (q % 4)) % n] for q in range(rp)]
        out.append(("rotation %d of %d" % (k, sets), tf, tp))
    return out


def schedule_coverage(t, scheds, p=pyref.P_PALLAS):
    """What a list of (targets_full, targets_partial) — the values the S-boxes really delivered — covers: bool arrays (corner, full round, element half)
    and (corner, q mod 4) over stored_corners(p), and the set of values that fill every slot of one schedule."""
    corners = stored_corners(p); idx = {c: i for i, c in enumerate(corners)}
    halves = element_halves(t)
    full = np.zeros((len(corners), len(scheds[0][0]), len(halves)), bool); part = np.zeros((len(corners), 4), bool); uniform = set()
    for tf, tp in scheds:
        for r, row in enumerate(tf):
            for h, (a, b) in enumerate(halves):
                for v in row[a:b]:
                    if v in idx:
                        full[idx[v], r, h] = True
        for q, v in enumerate(tp):
            if v in idx:
                part[idx[v], q % 4] = True
        vals = set(tp) | {v for row in tf for v in row}
        if len(vals) == 1:
            uniform |= vals
    return full, part, uniform


def node_digest(params, level, pos, label, stored_children, p=pyref.P_PALLAS):
    """pyref's hash_with_ds_dynamic of one Merkle node (DS words [arity, level, pos, label]) over stored children, as stored limbs"""
    Ri = pow(R, -1, p)
    kids = [raw_to_int(x) * Ri % p for x in np.asarray(stored_children, np.uint64).reshape(-1, 4)]
    return raw(pyref.hash_with_ds_dynamic([params["t"] - 1, level, pos, label], kids, params, p) * R % p)


def steered_set(params, sched, which, pos, level, label, count=None, p=pyref.P_PALLAS):
    """One steered set for the Merkle node at DS position `pos` ([arity, level, pos, label]) under the schedule `sched` = (name, targets_full,
    targets_partial).  which = 1: the first permutation of a node over `count` (default t - 1) stored corners as children; which = 2: both
    permutations of a full node (steered_node).  Returns a dict: the steered `params`, the node's stored `children`, its stored `digest`, the
    values `tf` / `tp` its S-boxes deliver, its first `state` (canonical), and the arguments."""
    t = params["t"]; arity = t - 1
    count = arity if count is None else count
    name, tf, tp = sched
    Ri = pow(R, -1, p); corners = stored_corners(p)
    given = [corners[(pos + 3 * j) % len(corners)] * Ri % p for j in range(count)]
    ds = [arity, level, pos, label]
    sp, kids, digest, tf2 = steered_node(params, ds, given, which, tf, tp, p)
    return dict(name=name, params=sp, children=to_stored(kids, p), digest=raw(digest * R % p), tf=tf2, tp=tp, state=first_state(params, ds, kids),
                which=which, pos=pos, level=level, label=label, count=count, t=t)


def steered_level(base, node, nodes, kstar, last_children=None, p=pyref.P_PALLAS):
    """(children, pos0): a crafted_level of `nodes` nodes under the base set's round-0 constants in which node kstar is the steered node of a
    steered_set.  The level starts at pos0 = pos - kstar: the constants are tied to the DS position, not to the index.  A node of fewer than
    t - 1 children can only be the ragged last one."""
    arity = base["t"] - 1
    ch, _ = crafted_level(base, nodes, p, last_children=last_children)
    assert node["count"] == (last_children if last_children is not None and kstar == nodes - 1 else arity) and 0 <= kstar < nodes and node["pos"] >= kstar
    ch[kstar * arity:kstar * arity + node["count"]] = node["children"]
    return ch, node["pos"] - kstar
