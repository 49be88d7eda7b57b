"""GPU: the wide Poseidon family h2_poseidon_wide_* (csrc/h2_poseidon.hpp, csrc/h2_poseidon_merkle.hpp) at widths 5 and 9 on all three scalar fields.

The judge is oracle/pyref.py (poseidon_permute, poseidon_hash_const_len with t = 5, 9); paths are judged by
poseidon.merkle_path_wide on a host copy of the tree and flipped paths by poseidon.hashn_int.  Every comparison is exact
equality of canonical values or of bytes.  Width 3 through the new entry points is compared with the old ones byte for
byte.  The references -- 257 permuted states, one tree per field and arity -- are computed once and shared; a smaller tree
is the front of the large one.  Outputs sit in front of a red zone filled with a pattern."""
import ctypes
import random

import numpy as np
import pytest

import pyref as R

pytestmark = pytest.mark.gpu

FIELD = {0: R.BN_FR, 1: R.PA_FQ, 2: R.PA_FP}
ROUNDS = {5: (8, 60), 9: (8, 63)}          # the Poseidon paper's numbers for these widths; the library fixes none
BIG = {5: 6, 9: 4}                         # 4096 leaves either way: a 1024- and a 512-node level above the tail threshold
H2_OK, H2_EINVAL = 0, -1
OK, RANGE, NONCANONICAL, MISMATCH = 0, 1, 2, 4
PATTERN = 0x5A5A5A5A5A5A5A5A
PATTERN32 = 0x5A5A5A5A
RED = 8
P = ctypes.c_void_p
CASES = [(cid, t) for cid in (0, 1, 2) for t in (5, 9)]


def L():
    from halo2_prover_amd import lib
    return lib.load()


def limbs(cid, values):
    return np.array([FIELD[cid].limbs(v) for v in values], dtype=np.uint64).reshape(-1, 4)


def raw_limbs(v):
    """the integer itself as four little-endian words (NOT Montgomery): how a non-canonical element is put in"""
    return np.array([(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)


def ints(cid, a):
    raw = np.ascontiguousarray(a).tobytes()
    return [FIELD[cid].from_mont(int.from_bytes(raw[i:i + 32], "little")) for i in range(0, len(raw), 32)]


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64).copy()).cuda()


def dev_u32(a):
    import torch
    return torch.from_numpy(np.array(a, dtype=np.uint32).view(np.int32).copy()).cuda()


def red_buffer(elems):
    import torch
    return torch.full((elems + RED, 4), PATTERN, dtype=torch.int64, device="cuda")


def red_status(n):
    import torch
    return torch.full((n + RED,), PATTERN32, dtype=torch.int32, device="cuda")


def split(buf, elems):
    h = buf.cpu().numpy().view(np.uint64)
    return h[:elems], bool((h[elems:] == PATTERN).all())


def split_status(buf, n):
    h = buf.cpu().numpy().view(np.uint32)
    return [int(x) for x in h[:n]], bool((h[n:] == PATTERN32).all())


def ptr(t):
    return None if t is None else P(t.data_ptr())


_CONST, _STATES, _TREE = {}, {}, {}


def consts(cid, t):
    if (cid, t) not in _CONST:
        _CONST[cid, t] = R.poseidon_constants(FIELD[cid], t, *ROUNDS[t])
    return _CONST[cid, t]


def ref_hash(cid, t, msg):
    rcs, mds = consts(cid, t)
    return R.poseidon_hash_const_len(FIELD[cid], msg, rcs, mds, *ROUNDS[t], t, t - 1)


def ref_states(cid, t):
    """257 states -- all zero, all p - 1, one of each, random -- and pyref's permutation of each, once per (field, width)"""
    if (cid, t) not in _STATES:
        f = FIELD[cid]
        rcs, mds = consts(cid, t)
        rnd = random.Random(0x51DE + 16 * cid + t)
        sts = [[0] * t, [f.p - 1] * t, [0] * (t - 1) + [f.p - 1], [f.p - 1] + [0] * (t - 1)]
        sts += [[rnd.randrange(f.p) for _ in range(t)] for _ in range(257 - len(sts))]
        _STATES[cid, t] = (sts, [R.poseidon_permute(f, s, rcs, mds, *ROUNDS[t]) for s in sts])
    return _STATES[cid, t]


def ref_tree(cid, t):
    """(leaves, levels) of one random tree of arity t - 1 and depth BIG[t] per field, by pyref, built once.  levels[l] are the
    nodes of level l (0: the leaves' parents).  The tree over the first a^d leaves is the front of every level"""
    if (cid, t) not in _TREE:
        a, p = t - 1, FIELD[cid].p
        rnd = random.Random(0x7EE5 + 16 * cid + t)
        leaves = [0, p - 1] + [rnd.randrange(p) for _ in range(a ** BIG[t] - 2)]
        levels, cur = [], leaves
        while len(cur) > 1:
            cur = [ref_hash(cid, t, cur[i:i + a]) for i in range(0, len(cur), a)]
            levels.append(cur)
        _TREE[cid, t] = (leaves, levels)
    return _TREE[cid, t]


def sub_tree(cid, t, depth):
    """(leaves, inner nodes in the device's order) of the tree over the first a^depth leaves of ref_tree"""
    a = t - 1
    leaves, levels = ref_tree(cid, t)
    nodes = []
    for l in range(depth):
        nodes += levels[l][:a ** (depth - 1 - l)]
    return leaves[:a ** depth], nodes


def device_tree(cid, t, depth):
    """the device's inner nodes of sub_tree's leaves, as limbs on the host, and the leaves' limbs"""
    a = t - 1
    leaf_limbs = limbs(cid, sub_tree(cid, t, depth)[0])
    count = (a ** depth - 1) // (a - 1)
    d_leaves, d_nodes = dev(leaf_limbs), red_buffer(count)
    assert L().h2_poseidon_wide_merkle_device(cid, t, *ROUNDS[t], ptr(d_leaves), depth, ptr(d_nodes), None) == H2_OK
    nodes, intact = split(d_nodes, count)
    assert intact
    return leaf_limbs, nodes.copy()


# ---- permute ------------------------------------------------------------------------------------------------------------
@pytest.fixture(params=[1, 2], ids=["dense", "sparse"])
def form(request):
    """the partial rounds of the permutation kernel for the length of a test"""
    assert L().h2_selftest_set_poseidon_wide_form(request.param) == H2_OK
    yield request.param
    assert L().h2_selftest_set_poseidon_wide_form(0) == H2_OK


@pytest.mark.parametrize("n", [1, 65, 257])
@pytest.mark.parametrize("cid,t", CASES)
def test_permute_equals_pyref_out_of_place_and_in_place(h2, form, cid, t, n):
    sts, want = ref_states(cid, t)
    a = limbs(cid, [x for s in sts[:n] for x in s])
    d_in, d_out = dev(a), red_buffer(n * t)
    assert L().h2_poseidon_wide_permute_device(cid, t, *ROUNDS[t], ptr(d_in), ptr(d_out), n, None) == H2_OK
    got, intact = split(d_out, n * t)
    assert intact and (d_in.cpu().numpy().view(np.uint64) == a).all()
    assert ints(cid, got) == [x for s in want[:n] for x in s]
    d_io = red_buffer(n * t)
    d_io[:n * t] = dev(a)
    assert L().h2_poseidon_wide_permute_device(cid, t, *ROUNDS[t], ptr(d_io), ptr(d_io), n, None) == H2_OK
    again, intact = split(d_io, n * t)
    assert intact and again.tobytes() == got.tobytes()


@pytest.mark.parametrize("cid,t", CASES)
def test_permute_through_the_python_layer_and_with_odd_rounds(h2, cid, t):
    """the width's own form, and an instance whose partial rounds end between two value reductions"""
    from halo2_prover_amd import poseidon
    sts, want = ref_states(cid, t)
    got = poseidon.permute(cid, limbs(cid, [x for s in sts[:3] for x in s]).reshape(3, t, 4), *ROUNDS[t], width=t)
    assert got.shape == (3, t, 4) and ints(cid, got) == [x for s in want[:3] for x in s]
    rcs, mds = R.poseidon_constants(FIELD[cid], t, 2, 11)
    got = poseidon.permute(cid, limbs(cid, sts[1] + sts[5]).reshape(2, t, 4), 2, 11, width=t)
    assert ints(cid, got) == [x for s in (sts[1], sts[5]) for x in R.poseidon_permute(FIELD[cid], s, rcs, mds, 2, 11)]
    with pytest.raises(ValueError):
        poseidon.permute(cid, limbs(cid, sts[0]).reshape(1, t, 4), width=t)        # no default rounds


# ---- hash ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", range(5))
@pytest.mark.parametrize("cid,t", CASES)
def test_hash_equals_pyref(h2, cid, t, which):
    rate = t - 1
    ln = (1, rate - 1, rate, rate + 1, 2 * rate + 1)[which]
    n, stride, p = 67, ln + 3, FIELD[cid].p
    rnd = random.Random(0xA5 + 100 * cid + 10 * t + which)
    rows = [[0] * stride, [p - 1] * stride] + [[rnd.randrange(p) for _ in range(stride)] for _ in range(n - 2)]
    d_msgs, d_out = dev(limbs(cid, [x for r in rows for x in r])), red_buffer(n)
    assert L().h2_poseidon_wide_hash_device(cid, t, *ROUNDS[t], ptr(d_msgs), ln, stride, n, ptr(d_out), None) == H2_OK
    got, intact = split(d_out, n)
    assert intact
    assert ints(cid, got) == [ref_hash(cid, t, r[:ln]) for r in rows]


@pytest.mark.parametrize("cid,t", [(1, 5), (0, 9)])
def test_hash_in_the_single_chain_form_and_through_the_python_layer(h2, cid, t):
    from halo2_prover_amd import poseidon
    rate, p = t - 1, FIELD[cid].p
    rnd = random.Random(0xC4A1 + t)
    rows = [[p - 1] * (rate + 1)] + [[rnd.randrange(p) for _ in range(rate + 1)] for _ in range(64)]
    want = [ref_hash(cid, t, r) for r in rows]
    a = limbs(cid, [x for r in rows for x in r]).reshape(len(rows), rate + 1, 4)
    try:
        for product_form in (1, 2):
            assert L().h2_selftest_set_poseidon_form(product_form) == H2_OK
            assert ints(cid, poseidon.hash(cid, a, *ROUNDS[t], width=t)) == want
    finally:
        assert L().h2_selftest_set_poseidon_form(0) == H2_OK
    assert ints(cid, poseidon.hash(cid, a, *ROUNDS[t], length=rate, width=t)) == [ref_hash(cid, t, r[:rate]) for r in rows]


# ---- width 3 through the new family ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,r_f,r_p", [(0, 8, 60), (1, 8, 56), (2, 8, 56)])
def test_width_3_is_the_old_family_byte_for_byte(h2, cid, r_f, r_p):
    lib, p = L(), FIELD[cid].p
    rnd = random.Random(0x333 + cid)
    vals = [0, p - 1] + [rnd.randrange(p) for _ in range(3 * 70 - 2)]
    a = limbs(cid, vals)
    d_in = dev(a)
    old, new = red_buffer(210), red_buffer(210)
    assert lib.h2_poseidon_permute_device(cid, r_f, r_p, ptr(d_in), ptr(old), 70, None) == H2_OK
    assert lib.h2_poseidon_wide_permute_device(cid, 3, r_f, r_p, ptr(d_in), ptr(new), 70, None) == H2_OK
    assert split(new, 210)[1] and split(new, 210)[0].tobytes() == split(old, 210)[0].tobytes()
    old, new = red_buffer(42), red_buffer(42)
    assert lib.h2_poseidon_hash_device(cid, r_f, r_p, ptr(d_in), 3, 5, 42, ptr(old), None) == H2_OK
    assert lib.h2_poseidon_wide_hash_device(cid, 3, r_f, r_p, ptr(d_in), 3, 5, 42, ptr(new), None) == H2_OK
    assert split(new, 42)[1] and split(new, 42)[0].tobytes() == split(old, 42)[0].tobytes()
    d_leaves = dev(a[:128])
    old, new = red_buffer(127), red_buffer(127)
    assert lib.h2_poseidon_merkle_device(cid, r_f, r_p, ptr(d_leaves), 7, ptr(old), None) == H2_OK
    assert lib.h2_poseidon_wide_merkle_device(cid, 3, r_f, r_p, ptr(d_leaves), 7, ptr(new), None) == H2_OK
    nodes, intact = split(new, 127)
    assert intact and nodes.tobytes() == split(old, 127)[0].tobytes()
    d_nodes, d_idx = dev(nodes), dev_u32([0, 127, 128, 77])
    po, pn, so, sn = red_buffer(28), red_buffer(28), red_status(4), red_status(4)
    assert lib.h2_poseidon_merkle_paths_device(cid, ptr(d_leaves), ptr(d_nodes), 7, ptr(d_idx), 4, ptr(po), ptr(so), None) == H2_OK
    assert lib.h2_poseidon_wide_merkle_paths_device(cid, 3, ptr(d_leaves), ptr(d_nodes), 7, ptr(d_idx), 4, ptr(pn), ptr(sn), None) == H2_OK
    assert split(pn, 28)[0].tobytes() == split(po, 28)[0].tobytes() and split_status(sn, 4) == split_status(so, 4) == ([0, 0, 1, 0], True)
    d_vals, d_root = dev(a[[0, 127, 5, 77]]), dev(nodes[-1:])
    ro, rn, so, sn = red_buffer(4), red_buffer(4), red_status(4), red_status(4)
    assert lib.h2_poseidon_merkle_verify_device(cid, r_f, r_p, ptr(d_vals), ptr(d_idx), ptr(pn), 7, 4, ptr(d_root), ptr(ro), ptr(so),
                                                None) == H2_OK
    assert lib.h2_poseidon_wide_merkle_verify_device(cid, 3, r_f, r_p, ptr(d_vals), ptr(d_idx), ptr(pn), 7, 4, ptr(d_root), ptr(rn),
                                                     ptr(sn), None) == H2_OK
    assert split(rn, 4)[0].tobytes() == split(ro, 4)[0].tobytes() and split_status(sn, 4) == split_status(so, 4) == ([0, 0, 1, 0], True)


# ---- Merkle trees ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,t,depth", [(cid, t, d) for cid in (0, 1, 2) for t, ds in ((5, (1, 2, 3, 6)), (9, (1, 2, 4))) for d in ds])
def test_merkle_equals_pyref(h2, cid, t, depth):
    """depth 6 / 4: a 1024- / 512-node level in a launch of its own, the rest in the tail; depths 1 .. 3: the tail alone,
    its first level narrower than a wave"""
    assert L().h2_poseidon_merkle_tail() == 256
    _, nodes = device_tree(cid, t, depth)
    assert ints(cid, nodes) == sub_tree(cid, t, depth)[1]


@pytest.mark.parametrize("t,tail", [(5, 4), (5, 512), (9, 512), (9, 8)])
def test_merkle_with_the_tail_threshold_moved(h2, t, tail):
    """512 (a power of 8, not of 4): a lane of the tail hashes two nodes of the 512-node level; 4 and 8: every wider level is a launch"""
    lib = L()
    try:
        assert lib.h2_selftest_set_poseidon_merkle_tail(tail) == H2_OK
        _, nodes = device_tree(1, t, BIG[t])
    finally:
        assert lib.h2_selftest_set_poseidon_merkle_tail(0) == H2_OK
    assert ints(1, nodes) == sub_tree(1, t, BIG[t])[1]


def test_merkle_through_the_python_layer(h2):
    from halo2_prover_amd import poseidon
    leaves, nodes = sub_tree(2, 5, 2)
    got = poseidon.merkle_nodes("vesta", limbs(2, leaves), *ROUNDS[5], width=5)
    assert got.shape == (5, 4) and ints(2, got) == nodes
    assert ints(2, poseidon.merkle_root("vesta", limbs(2, leaves), *ROUNDS[5], width=5)) == nodes[-1:]
    with pytest.raises(ValueError):
        poseidon.merkle_nodes("vesta", limbs(2, leaves[:8]), *ROUNDS[5], width=5)       # 8 is no power of 4


# ---- paths and verify -------------------------------------------------------------------------------------------------------
def indices_33(t, depth, rnd):
    a = t - 1
    return [0, a ** depth - 1, a ** depth, 1, a - 1, a] + [rnd.randrange(a ** depth) for _ in range(27)]


@pytest.mark.parametrize("cid,t", CASES)
def test_paths_and_verify(h2, cid, t):
    from halo2_prover_amd import poseidon
    lib, a, depth, p = L(), t - 1, BIG[t], FIELD[cid].p
    per = depth * (a - 1)
    leaves, want_nodes = sub_tree(cid, t, depth)
    leaf_limbs, node_limbs = device_tree(cid, t, depth)
    whole = leaves + want_nodes
    root = whole[-1]
    idx = indices_33(t, depth, random.Random(0x1D + cid + t))
    n = len(idx)
    d_leaves, d_nodes, d_idx = dev(leaf_limbs), dev(node_limbs), dev_u32(idx)
    d_paths, d_st = red_buffer(n * per), red_status(n)
    assert lib.h2_poseidon_wide_merkle_paths_device(cid, t, ptr(d_leaves), ptr(d_nodes), depth, ptr(d_idx), n, ptr(d_paths), ptr(d_st),
                                                    None) == H2_OK
    paths, intact = split(d_paths, n * per)
    st, st_intact = split_status(d_st, n)
    assert intact and st_intact and st == [RANGE if i >= a ** depth else OK for i in idx]
    got = ints(cid, paths)
    for j, i in enumerate(idx):
        want = [0] * per if i >= a ** depth else poseidon.merkle_path_wide(whole, a, depth, i)
        assert got[j * per:(j + 1) * per] == want, (j, i)
    assert not paths[2 * per:3 * per].any()                      # the item out of range: zero bytes, not a zero element

    def verify(values, path_limbs, d_root, want_roots=True):
        d_vals, d_p = dev(values), dev(path_limbs)
        d_r, d_s = (red_buffer(n) if want_roots else None), red_status(n)
        assert lib.h2_poseidon_wide_merkle_verify_device(cid, t, *ROUNDS[t], ptr(d_vals), ptr(d_idx), ptr(d_p), depth, n, ptr(d_root),
                                                         ptr(d_r), ptr(d_s), None) == H2_OK
        s, ok = split_status(d_s, n)
        assert ok
        if not want_roots:
            return None, s
        r, ok = split(d_r, n)
        assert ok
        return r.reshape(n, 4), s

    values = np.stack([leaf_limbs[i] if i < a ** depth else leaf_limbs[0] for i in idx])
    d_root = dev(limbs(cid, [root]))
    roots, st = verify(values, paths, d_root)
    assert st == [RANGE if i >= a ** depth else OK for i in idx]
    assert not roots[2].any() and ints(cid, np.delete(roots, 2, axis=0)) == [root] * (n - 1)
    assert verify(values, paths, d_root, want_roots=False)[1] == st

    # item 3: a sibling of the second level flipped; item 4: another leaf value; 5: a sibling >= p; 6: a leaf value >= p;
    # 7: the LAST sibling = p exactly
    bad_paths, bad_values = paths.reshape(n, per, 4).copy(), values.copy()
    flipped = poseidon.merkle_path_wide(whole, a, depth, idx[3])
    flipped[a] = (flipped[a] + 1) % p
    bad_paths[3] = limbs(cid, flipped)
    bad_values[4] = limbs(cid, [(leaves[idx[4]] + 1) % p])[0]
    bad_paths[5][1] = raw_limbs(p + 5)
    bad_values[6] = raw_limbs((1 << 256) - 1)
    bad_paths[7][per - 1] = raw_limbs(p)
    roots, st = verify(bad_values, bad_paths.reshape(n * per, 4), d_root)
    assert st[:8] == [OK, OK, RANGE, MISMATCH, MISMATCH, NONCANONICAL, NONCANONICAL, NONCANONICAL] and st[8:] == [OK] * (n - 8)
    for j in (2, 5, 6, 7):
        assert not roots[j].any()

    def walk(leaf, index, path):
        for l in range(depth):
            sibs = list(path[l * (a - 1):(l + 1) * (a - 1)])
            sibs.insert(index % a, leaf)
            leaf, index = poseidon.hashn_int(cid, sibs, *ROUNDS[t]), index // a
        return leaf

    assert ints(cid, roots[3]) == [walk(leaves[idx[3]], idx[3], flipped)] != [root]
    assert ints(cid, roots[4]) == [walk((leaves[idx[4]] + 1) % p, idx[4], poseidon.merkle_path_wide(whole, a, depth, idx[4]))]
    # no root to compare with: the mismatches are gone, the computed roots stay
    roots2, st = verify(bad_values, bad_paths.reshape(n * per, 4), None)
    assert st[:8] == [OK, OK, RANGE, OK, OK, NONCANONICAL, NONCANONICAL, NONCANONICAL] and roots2.tobytes() == roots.tobytes()


def test_paths_and_verify_through_the_python_layer(h2):
    from halo2_prover_amd import poseidon
    cid, t, depth = 1, 9, 2
    leaves, nodes = sub_tree(cid, t, depth)
    leaf_limbs, node_limbs = limbs(cid, leaves), limbs(cid, nodes)
    idx = np.array([0, 63, 64, 9], dtype=np.uint32)
    paths, st = poseidon.merkle_paths(cid, leaf_limbs, node_limbs, idx, width=t)
    assert paths.shape == (4, 14, 4) and list(st) == [0, 0, 1, 0]
    assert ints(cid, paths[3]) == poseidon.merkle_path_wide(leaves + nodes, 8, depth, 9)
    roots, st = poseidon.verify_paths(cid, leaf_limbs[[0, 63, 0, 9]], idx, paths, limbs(cid, nodes[-1:]), *ROUNDS[t], width=t)
    assert list(st) == [0, 0, 1, 0] and ints(cid, roots[[0, 1, 3]]) == nodes[-1:] * 3
    assert poseidon.verify_path_wide(cid, 8, leaves[9], 9, ints(cid, paths[3]), nodes[-1], *ROUNDS[t])
    empty = np.zeros((0,), dtype=np.uint32)
    paths, st = poseidon.merkle_paths(cid, leaf_limbs, node_limbs, empty, width=t)
    assert paths.shape == (0, 14, 4) and st.shape == (0,)


# ---- argument checks --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", [5, 9])
def test_invalid_arguments_are_refused_and_nothing_is_written(h2, t):
    import torch
    lib, cid, a = L(), 1, t - 1
    r_f, r_p = ROUNDS[t]
    depth, n = 2, 3
    leaves, nodes = a ** depth, a + 1
    per = depth * (a - 1)
    buf = red_buffer(4 * leaves + 64)          # one allocation: ranges inside it can be made to overlap
    base = buf.data_ptr()
    at = lambda e: P(base + 32 * e)            # noqa: E731 -- element e of the buffer
    st = red_status(16)
    st_at = lambda w: P(st.data_ptr() + 4 * w)  # noqa: E731
    d_idx = dev_u32([0, 1, 2, 3])
    i_ptr, L0, N0, OUT, PATHS = ptr(d_idx), 0, leaves, 2 * leaves, 3 * leaves    # leaves, nodes, outputs, verify's paths in buf
    calls = {
        "permute": lambda **k: lib.h2_poseidon_wide_permute_device(k.get("cid", cid), k.get("t", t), k.get("r_f", r_f), r_p,
                                                                   k.get("i", at(L0)), k.get("o", at(OUT)), k.get("n", n), None),
        "hash": lambda **k: lib.h2_poseidon_wide_hash_device(k.get("cid", cid), k.get("t", t), k.get("r_f", r_f), r_p, k.get("i", at(L0)),
                                                             k.get("len", a), k.get("stride", a), k.get("n", n), k.get("o", at(OUT)), None),
        "merkle": lambda **k: lib.h2_poseidon_wide_merkle_device(k.get("cid", cid), k.get("t", t), k.get("r_f", r_f), r_p,
                                                                 k.get("i", at(L0)), k.get("depth", depth), k.get("o", at(N0)), None),
        "paths": lambda **k: lib.h2_poseidon_wide_merkle_paths_device(k.get("cid", cid), k.get("t", t), k.get("i", at(L0)), at(N0),
                                                                      k.get("depth", depth), k.get("idx", i_ptr), k.get("n", n),
                                                                      k.get("o", at(OUT)), k.get("st", st_at(0)), None),
        "verify": lambda **k: lib.h2_poseidon_wide_merkle_verify_device(k.get("cid", cid), k.get("t", t), k.get("r_f", r_f), r_p,
                                                                        k.get("i", at(L0)), k.get("idx", i_ptr), k.get("p", at(PATHS)),
                                                                        k.get("depth", depth), k.get("n", n), k.get("root", None),
                                                                        k.get("o", at(OUT)), k.get("st", st_at(0)), None),
    }
    bad = [(name, kw) for name in calls for kw in ({"cid": 3}, {"t": 4}, {"t": 7}, {"i": P(base + 8)}, {"o": P(base + 32 * OUT + 4)},
                                                   {"i": None}, {"o": None} if name != "verify" else {"st": None})]
    bad += [(name, {"r_f": 7}) for name in ("permute", "hash", "merkle", "verify")]
    bad += [(name, {"depth": 0}) for name in ("merkle", "paths", "verify")]
    bad += [(name, {"depth": 30 // (2 if t == 5 else 3) + 1}) for name in ("merkle", "paths", "verify")]      # a^depth > 2^30
    bad += [("permute", {"o": at(L0 + 1)}), ("permute", {"n": (1 << 40) + 1}), ("hash", {"len": 0}), ("hash", {"stride": a - 1}),
            ("hash", {"len": 65536, "stride": 65536}), ("hash", {"o": at(L0 + 2)}), ("merkle", {"o": at(L0 + leaves - 1)}),
            ("paths", {"o": at(N0 + nodes - 1)}), ("paths", {"o": at(L0 + leaves - 1)}), ("paths", {"st": P(d_idx.data_ptr())}),
            ("paths", {"n": (1 << 31) + 1}), ("verify", {"o": at(PATHS + n * per - 1)}), ("verify", {"o": at(L0 + n - 1)}),
            ("verify", {"root": at(OUT + 1)}), ("verify", {"root": P(base + 4)}), ("verify", {"o": P(base + 32 * OUT + 8)}),
            ("verify", {"st": P(d_idx.data_ptr() + 8)})]
    for name, kw in bad:
        assert calls[name](**kw) == H2_EINVAL, (name, kw)
    for name in calls:                          # n = 0: fine, and nothing is enqueued
        if name != "merkle":
            assert calls[name](n=0) == H2_OK, name
    torch.cuda.synchronize()
    assert (buf.cpu().numpy().view(np.uint64) == PATTERN).all() and (st.cpu().numpy().view(np.uint32) == PATTERN32).all()
    assert (d_idx.cpu().numpy().view(np.uint32) == [0, 1, 2, 3]).all()
    # every call as it stands is accepted (so each refusal above is due to the one argument changed), d_out == d_in too
    for name in calls:
        assert calls[name]() == H2_OK, name
    assert calls["permute"](i=at(OUT)) == H2_OK
    torch.cuda.synchronize()
