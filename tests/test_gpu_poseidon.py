"""GPU: h2_poseidon_permute_device / h2_poseidon_hash_device / h2_poseidon_merkle_device (csrc/h2_poseidon.hpp).

The judge is oracle/pyref.py (poseidon_constants, poseidon_permute, poseidon_hash_const_len) on Python integers, and the
zcash vectors of tests/golden/pasta_poseidon_vectors.json (`fp` is Vesta's scalar field, curve 2; `fq` is Pallas's, curve
1).  Every comparison is exact equality of canonical values.  The references are computed once per field and shared: the
permutations of one list of states, and ONE tree of 2^11 leaves -- the tree over the first 2^d leaves is a sub-tree of it.

Outputs sit in front of a red zone filled with a pattern: whatever a call was not asked to write comes back unchanged."""
import ctypes
import json
import os
import random

import numpy as np
import pytest

import pyref as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIELD = {0: R.BN_FR, 1: R.PA_FQ, 2: R.PA_FP}
JSON_NAME = {1: "fq", 2: "fp"}
SPEC = {0: (8, 60), 1: (8, 56), 2: (8, 56)}
H2_OK, H2_EINVAL = 0, -1
PATTERN = 0x5A5A5A5A5A5A5A5A
RED = 8                                   # elements of PATTERN behind an output
POSEIDON_1_2 = 0x152E960B5C9C8A624B2CDF4855250E8A54EE074254281310DC4A9704F78C1917
MAX_DEPTH = 11


def L():
    from halo2_prover_amd import lib
    return lib.load()


def le(hexstr):
    return int.from_bytes(bytes.fromhex(hexstr), "little")


def vectors():
    return json.load(open(os.path.join(GOLDEN, "pasta_poseidon_vectors.json")))


def limbs(cid, values):
    return np.array([FIELD[cid].limbs(v) for v in values], dtype=np.uint64).reshape(-1, 4)


def ints(cid, a):
    raw = np.ascontiguousarray(a).tobytes()
    return [FIELD[cid].from_mont(int.from_bytes(raw[i:i + 32], "little")) for i in range(0, len(raw), 32)]


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64).copy()).cuda()


def red_buffer(elems):
    """`elems` elements for an output and RED more, all of it the pattern"""
    import torch
    return torch.full((elems + RED, 4), PATTERN, dtype=torch.int64, device="cuda")


def split(buf, elems):
    """(the output's limbs, True if the red zone is intact)"""
    h = buf.cpu().numpy().view(np.uint64)
    return h[:elems], bool((h[elems:] == PATTERN).all())


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


_CONST, _PERM, _TREE = {}, {}, {}


def ref_constants(cid, r_f, r_p):
    key = (cid, r_f, r_p)
    if key not in _CONST:
        _CONST[key] = R.poseidon_constants(FIELD[cid], 3, r_f, r_p)
    return _CONST[key]


def ref_hash(cid, msg, r_f, r_p):
    rcs, mds = ref_constants(cid, r_f, r_p)
    return R.poseidon_hash_const_len(FIELD[cid], msg, rcs, mds, r_f, r_p)


def ref_states(cid):
    """257 states, the extremes first, and their permutations under the field's spec (once per field)"""
    if cid not in _PERM:
        f = FIELD[cid]
        r_f, r_p = SPEC[cid]
        rcs, mds = ref_constants(cid, r_f, r_p)
        rnd = random.Random(0x57A7E + cid)
        states = [[0, 0, 0], [f.p - 1] * 3, [0, f.p - 1, 1]] + [[rnd.randrange(f.p) for _ in range(3)] for _ in range(254)]
        _PERM[cid] = (states, [R.poseidon_permute(f, s, rcs, mds, r_f, r_p) for s in states])
    return _PERM[cid]


def ref_tree(cid):
    """2^11 leaves and the levels above them, level by level (once per field)"""
    if cid not in _TREE:
        f = FIELD[cid]
        r_f, r_p = SPEC[cid]
        rnd = random.Random(0x7EE + cid)
        leaves = [0, f.p - 1] + [rnd.randrange(f.p) for _ in range((1 << MAX_DEPTH) - 2)]
        levels = [leaves]
        while len(levels[-1]) > 1:
            lo = levels[-1]
            levels.append([ref_hash(cid, lo[2 * i:2 * i + 2], r_f, r_p) for i in range(len(lo) // 2)])
        _TREE[cid] = levels
    return _TREE[cid]


def permute_raw(cid, r_f, r_p, states, stream=None):
    """states: ints (n, 3) -> (result ints, red zone intact)"""
    n = len(states)
    d_in = dev(limbs(cid, [x for s in states for x in s]))
    d_out = red_buffer(3 * n)
    assert L().h2_poseidon_permute_device(cid, r_f, r_p, ptr(d_in), ptr(d_out), n, stream) == H2_OK
    out, intact = split(d_out, 3 * n)
    v = ints(cid, out)
    return [v[3 * i:3 * i + 3] for i in range(n)], intact


def hash_raw(cid, r_f, r_p, msgs, stride=None):
    """msgs: n lists of len ints, laid out `stride` elements apart with the pattern in the gaps"""
    n, ln = len(msgs), len(msgs[0])
    stride = ln if stride is None else stride
    host = np.full((n * stride, 4), PATTERN, dtype=np.uint64)
    for i, m in enumerate(msgs):
        host[i * stride:i * stride + ln] = limbs(cid, m)
    d_in = dev(host)
    d_out = red_buffer(n)
    assert L().h2_poseidon_hash_device(cid, r_f, r_p, ptr(d_in), ln, stride, n, ptr(d_out), None) == H2_OK
    out, intact = split(d_out, n)
    return ints(cid, out), intact


# ---- permute ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [1, 2])
def test_permute_the_vectors_in_one_call(h2, cid):
    v = vectors()[JSON_NAME[cid]]["permute"]
    assert len(v) == 11
    got, intact = permute_raw(cid, 8, 56, [[le(x) for x in t["initial_state"]] for t in v])
    assert got == [[le(x) for x in t["final_state"]] for t in v] and intact


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("cid", [0, 1, 2])
def test_permute_random_states_and_the_extremes(h2, cid, n):
    states, want = ref_states(cid)
    got, intact = permute_raw(cid, *SPEC[cid], states[:n])
    assert got == want[:n]
    assert intact, "the pattern behind the last output state was overwritten"


def test_permute_in_place(h2):
    cid = 2
    states, want = ref_states(cid)
    n = 65
    buf = red_buffer(3 * n)
    buf[:3 * n] = dev(limbs(cid, [x for s in states[:n] for x in s]))
    assert L().h2_poseidon_permute_device(cid, 8, 56, ptr(buf), ptr(buf), n, None) == H2_OK
    out, intact = split(buf, 3 * n)
    v = ints(cid, out)
    assert [v[3 * i:3 * i + 3] for i in range(n)] == want[:n] and intact


def test_permute_nothing(h2):
    buf = red_buffer(3)
    assert L().h2_poseidon_permute_device(1, 8, 56, ptr(buf), ptr(buf), 0, None) == H2_OK
    assert split(buf, 0)[1]


def test_permute_on_another_stream_through_the_python_layer(h2):
    import torch
    from halo2_prover_amd import poseidon
    cid = 0
    states, want = ref_states(cid)
    n = 65
    s = torch.cuda.Stream()
    d_in = dev(limbs(cid, [x for st in states[:n] for x in st])).reshape(n, 3, 4)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        d_out = poseidon.permute("bn254", d_in)
    s.synchronize()
    v = ints(cid, d_out.cpu().numpy().view(np.uint64))
    assert [v[3 * i:3 * i + 3] for i in range(n)] == want[:n]
    # numpy in, numpy out
    got = poseidon.permute(cid, limbs(cid, [x for st in states[:3] for x in st]).reshape(3, 3, 4))
    assert isinstance(got, np.ndarray) and ints(cid, got) == [x for st in want[:3] for x in st]


# ---- hash -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [1, 2])
def test_hash_the_vectors(h2, cid):
    v = vectors()[JSON_NAME[cid]]["hash"]
    assert len(v) == 11
    got, intact = hash_raw(cid, 8, 56, [[le(x) for x in t["input"]] for t in v])
    assert got == [le(t["output"]) for t in v] and intact


def test_hash_one_two_on_bn254(h2):
    assert hash_raw(0, 8, 60, [[1, 2]]) == ([POSEIDON_1_2], True)


@pytest.mark.parametrize("n", [1, 65])
@pytest.mark.parametrize("ln", [1, 2, 3, 4, 5])
def test_hash_lengths_cover_the_pad_and_several_absorbs(h2, ln, n):
    cid = 1 + (ln & 1)
    f = FIELD[cid]
    rnd = random.Random(100 * ln + n)
    msgs = [[0] * ln, [f.p - 1] * ln][:n] + [[rnd.randrange(f.p) for _ in range(ln)] for _ in range(max(0, n - 2))]
    got, intact = hash_raw(cid, 8, 56, msgs)
    assert got == [ref_hash(cid, m, 8, 56) for m in msgs] and intact


@pytest.mark.parametrize("ln", [1, 2, 5])
def test_hash_strided_messages(h2, ln):
    cid = 0
    rnd = random.Random(7 + ln)
    msgs = [[rnd.randrange(FIELD[cid].p) for _ in range(ln)] for _ in range(65)]
    got, intact = hash_raw(cid, 8, 60, msgs, stride=ln + 3)
    assert got == [ref_hash(cid, m, 8, 60) for m in msgs] and intact


def test_hash_with_other_round_counts(h2):
    """nothing is hard-wired to the two specs"""
    cid = 2
    rnd = random.Random(43)
    msgs = [[rnd.randrange(FIELD[cid].p) for _ in range(3)] for _ in range(5)]
    got, intact = hash_raw(cid, 4, 3, msgs)
    assert got == [ref_hash(cid, m, 4, 3) for m in msgs] and intact


def test_hash_through_the_python_layer(h2):
    from halo2_prover_amd import poseidon
    cid = 1
    msgs = [[3, 4, 5], [6, 7, 8]]
    arr = limbs(cid, [x for m in msgs for x in m]).reshape(2, 3, 4)
    assert ints(cid, poseidon.hash("pallas", arr)) == [ref_hash(cid, m, 8, 56) for m in msgs]
    assert ints(cid, poseidon.hash("pallas", arr, length=2)) == [ref_hash(cid, m[:2], 8, 56) for m in msgs]
    assert ints(0, poseidon.hash("bn254", limbs(0, [1, 2]).reshape(1, 2, 4))) == [POSEIDON_1_2]


# ---- merkle -----------------------------------------------------------------------------------------------------------
def merkle_depths():
    t = L().h2_poseidon_merkle_tail()
    lt = t.bit_length() - 1
    assert t == 1 << lt and lt + 2 < MAX_DEPTH, "the depths below no longer straddle the tail width"
    return sorted({1, 2, lt, lt + 1, lt + 2, MAX_DEPTH} - {0})


@pytest.mark.parametrize("which", range(6))
@pytest.mark.parametrize("cid", [0, 1])
def test_merkle_all_nodes(h2, cid, which):
    """tail only (depth <= log2 T + 1), exactly one level launch (log2 T + 2), two (11)"""
    depths = merkle_depths()
    depth = depths[min(which, len(depths) - 1)]
    levels = ref_tree(cid)
    n = 1 << depth
    want = [x for lv in range(1, depth + 1) for x in levels[lv][:n >> lv]]
    assert len(want) == n - 1
    d_leaves = dev(limbs(cid, levels[0][:n]))
    d_nodes = red_buffer(n - 1)
    assert L().h2_poseidon_merkle_device(cid, *SPEC[cid], ptr(d_leaves), depth, ptr(d_nodes), None) == H2_OK
    out, intact = split(d_nodes, n - 1)
    assert ints(cid, out) == want
    assert intact, "the pattern behind d_nodes was overwritten"


def test_merkle_through_the_python_layer_and_a_membership_proof(h2):
    from halo2_prover_amd import poseidon
    cid, depth = 1, 4
    levels = ref_tree(cid)
    n = 1 << depth
    leaves = levels[0][:n]
    nodes = ints(cid, poseidon.merkle_nodes("pallas", limbs(cid, leaves)))
    assert nodes[-1] == levels[depth][0]
    assert ints(cid, poseidon.merkle_root(cid, dev(limbs(cid, leaves))).cpu().numpy().view(np.uint64)) == [nodes[-1]]
    path = poseidon.merkle_path(leaves + nodes, depth, 5)
    assert poseidon.verify_path(cid, leaves[5], 5, path, nodes[-1])
    assert not poseidon.verify_path(cid, leaves[4], 5, path, nodes[-1])


# ---- the table cache --------------------------------------------------------------------------------------------------
def test_nine_instances_in_a_row_then_the_first_again(h2):
    """the cache holds eight tables: the ninth drops the first, which is then built again"""
    cid = 2
    msgs = [[1, 2], [FIELD[cid].p - 1, 0], [3, 4]]
    pairs = [(2, k) for k in range(9)] + [(2, 0)]
    for r_f, r_p in pairs:
        got, intact = hash_raw(cid, r_f, r_p, msgs)
        assert got == [ref_hash(cid, m, r_f, r_p) for m in msgs] and intact, (r_f, r_p)


# ---- errors: H2_EINVAL on the host, nothing written ---------------------------------------------------------------------
def test_invalid_arguments_are_refused_and_nothing_is_written(h2):
    lib = L()
    src = dev(limbs(1, list(range(1, 65))))
    out = red_buffer(64)
    a, o = src.data_ptr(), out.data_ptr()
    P = ctypes.c_void_p
    bad_permute = [
        (1, 7, 56, P(a), P(o), 4), (1, 0, 56, P(a), P(o), 4), (1, 8, 121, P(a), P(o), 4), (3, 8, 56, P(a), P(o), 4),
        (1, 8, 56, None, P(o), 4), (1, 8, 56, P(a), None, 4), (1, 8, 56, P(a + 8), P(o), 4), (1, 8, 56, P(a), P(o + 8), 4),
        (1, 8, 56, P(a), P(a + 96), 4),                 # partial overlap
    ]
    for args in bad_permute:
        assert lib.h2_poseidon_permute_device(*args, None) == H2_EINVAL, args
    bad_hash = [
        (1, 8, 56, P(a), 0, 2, 4, P(o)), (1, 8, 56, P(a), 65536, 65536, 1, P(o)), (1, 8, 56, P(a), 3, 2, 4, P(o)),
        (1, 9, 56, P(a), 2, 2, 4, P(o)), (1, 8, 56, None, 2, 2, 4, P(o)), (1, 8, 56, P(a), 2, 2, 4, None),
        (1, 8, 56, P(a + 4), 2, 2, 4, P(o)), (1, 8, 56, P(a), 2, 2, 4, P(a + 32)), (7, 8, 56, P(a), 2, 2, 4, P(o)),
    ]
    for args in bad_hash:
        assert lib.h2_poseidon_hash_device(*args, None) == H2_EINVAL, args
    bad_merkle = [
        (1, 8, 56, P(a), 0, P(o)), (1, 8, 56, P(a), 31, P(o)), (1, 8, 57, P(a), 31, P(o)), (1, 3, 56, P(a), 2, P(o)),
        (1, 8, 56, None, 2, P(o)), (1, 8, 56, P(a), 2, None), (1, 8, 56, P(a), 2, P(o + 2)), (1, 8, 56, P(a), 2, P(a + 64)),
    ]
    for args in bad_merkle:
        assert lib.h2_poseidon_merkle_device(*args, None) == H2_EINVAL, args
    assert lib.h2_poseidon_hash_device(1, 8, 56, P(a), 2, 2, 0, P(o), None) == H2_OK          # n = 0: nothing enqueued
    assert split(out, 0)[1], "a refused call wrote to its output"
    assert ints(1, src.cpu().numpy().view(np.uint64)) == list(range(1, 65))


# ---- the two product forms of the hash kernel ---------------------------------------------------------------------------
CHAIN_MIN_N = (1 << 16) + 1            # csrc/h2_poseidon.hpp: a hash launch of this many lanes takes the single-chain products


@pytest.fixture
def form():
    """h2_selftest_set_poseidon_form for the length of a test: 1 = the compiler's products, 2 = single-chain, 0 = by size"""
    yield lambda which: L().h2_selftest_set_poseidon_form(which)
    assert L().h2_selftest_set_poseidon_form(0) == H2_OK


@pytest.mark.parametrize("cid", [0, 1])
def test_hash_on_both_sides_of_the_size_where_the_product_form_changes(h2, form, cid):
    """n = the threshold - 1 and the threshold + 64: the choice by size, and each form forced, give the same elements; a
    sample of them, the ends included, equals pyref (65 601 big-integer hashes would take half a minute)"""
    import torch
    f = FIELD[cid]
    r_f, r_p = SPEC[cid]
    n = CHAIN_MIN_N + 64
    g = torch.Generator(device="cuda")
    g.manual_seed(11 + cid)
    msgs = torch.randint(0, 1 << 62, (2 * n, 4), dtype=torch.int64, device="cuda", generator=g)
    msgs[:, 3] &= (1 << 61) - 1                       # below 2^253: canonical in all three fields
    assert form(3) == H2_EINVAL
    outs = {}
    for which, count in ((0, n), (1, n), (2, n), (0, CHAIN_MIN_N - 1)):
        assert form(which) == H2_OK
        d_out = red_buffer(count)
        assert L().h2_poseidon_hash_device(cid, r_f, r_p, ptr(msgs), 2, 2, count, ptr(d_out), None) == H2_OK
        out, intact = split(d_out, count)
        assert intact
        outs[(which, count)] = out
    assert np.array_equal(outs[(0, n)], outs[(1, n)]) and np.array_equal(outs[(0, n)], outs[(2, n)])
    assert np.array_equal(outs[(0, n)][:CHAIN_MIN_N - 1], outs[(0, CHAIN_MIN_N - 1)])
    rnd = random.Random(5)
    sample = [0, 1, 255, 256, CHAIN_MIN_N - 2, CHAIN_MIN_N - 1, CHAIN_MIN_N, n - 1] + [rnd.randrange(n) for _ in range(24)]
    host = msgs.cpu().numpy().view(np.uint64)
    for i in sample:
        m = ints(cid, host[2 * i:2 * i + 2])
        assert ints(cid, outs[(0, n)][i]) == [ref_hash(cid, m, r_f, r_p)], i


@pytest.mark.parametrize("which", [1, 2])
def test_merkle_level_launches_on_either_product_form(h2, form, which):
    cid, depth = 1, MAX_DEPTH
    levels = ref_tree(cid)
    want = [x for lv in range(1, depth + 1) for x in levels[lv]]
    assert form(which) == H2_OK
    d_nodes = red_buffer((1 << depth) - 1)
    assert L().h2_poseidon_merkle_device(cid, 8, 56, ptr(dev(limbs(cid, levels[0]))), depth, ptr(d_nodes), None) == H2_OK
    out, intact = split(d_nodes, (1 << depth) - 1)
    assert ints(cid, out) == want and intact


def test_merkle_with_other_tail_widths(h2):
    """the widths of the sweep in tools/poseidon_bench.py, the widest (two nodes per lane of the tail) included"""
    cid, depth = 0, 10
    levels = ref_tree(cid)
    n = 1 << depth
    want = [x for lv in range(1, depth + 1) for x in levels[lv][:n >> lv]]
    d_leaves = dev(limbs(cid, levels[0][:n]))
    try:
        assert L().h2_selftest_set_poseidon_merkle_tail(3) == H2_EINVAL and L().h2_selftest_set_poseidon_merkle_tail(1024) == H2_EINVAL
        for t in (1, 32, 512):
            assert L().h2_selftest_set_poseidon_merkle_tail(t) == H2_OK and L().h2_poseidon_merkle_tail() == t
            d_nodes = red_buffer(n - 1)
            assert L().h2_poseidon_merkle_device(cid, 8, 60, ptr(d_leaves), depth, ptr(d_nodes), None) == H2_OK
            out, intact = split(d_nodes, n - 1)
            assert ints(cid, out) == want and intact, t
    finally:
        assert L().h2_selftest_set_poseidon_merkle_tail(0) == H2_OK


# ---- the first user: h2_verify_proofs hashes a Poseidon batch's public inputs in one launch -------------------------------
def test_batch_verifier_with_device_hashes_agrees_with_the_single_verifier(h2):
    """three Poseidon k = 6 proofs made by h2_generate_proofs, one presented with a tampered message: with the threshold at
    2 the batch takes the device route, and ok[i] must be what h2_verify_proof says about item i alone"""
    import json as _json
    from test_capi_product import GOLDEN as G, c_verify, golden
    from test_gpu_prove_batch import c_prove_batch, streams_rng
    from test_gpu_verify_batch import c_verify_batch
    lib = L()
    params = golden("params_k6.bin")
    jsons = _json.load(open(os.path.join(G, "prove_batch_pins.json")))["poseidon"]["inputs"][:3]
    cb, ctxs = streams_rng(3)
    rc, proofs, _, _, _ = c_prove_batch(lib, params, jsons, 2, cb, ctxs)
    assert rc == H2_OK
    item = _json.loads(jsons[1])
    tampered = '{"x":[%d,%d],"output":"%s"}' % (item["x"][0], item["x"][1] + 1, item["output"])
    items = [(proofs[0], jsons[0]), (proofs[1], tampered), (proofs[2], jsons[2])]
    singles = [c_verify(lib, params, p, js, 2) for p, js in items]
    assert singles == [(0, 1), (0, 0), (0, 1)]
    try:
        assert lib.h2_selftest_set_poseidon_verify_min(2) == H2_OK
        rc, ok, all_ok = c_verify_batch(lib, params, items, 2)
        assert (rc, ok, all_ok) == (H2_OK, [s[1] for s in singles], 0)
        rc, ok, all_ok = c_verify_batch(lib, params, [items[0], items[2]], 2)
        assert (rc, ok, all_ok) == (H2_OK, [1, 1], 1)
        assert lib.h2_selftest_set_poseidon_verify_min(4) == H2_OK          # below the threshold: the host route, the same answers
        rc, ok, all_ok = c_verify_batch(lib, params, items, 2)
        assert (rc, ok, all_ok) == (H2_OK, [1, 0, 1], 0)
    finally:
        assert lib.h2_selftest_set_poseidon_verify_min(0) == H2_OK
