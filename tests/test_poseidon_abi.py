"""CPU (no GPU): the ABI of h2_poseidon_* -- exported, listed by the loader, declared in the header, h2_version() unmoved --
the constant generation against oracle/pyref.py and the reference's recorded values, and the HOST instantiation of the
kernels' permutation template (h2_selftest_poseidon) against the 44 zcash vectors, the recorded bn256 hash and pyref on
the extremes of the bound analysis.  Every comparison is exact equality of canonical values.

Which field goes with which curve: the JSON's `fp` is Vesta's scalar field (curve 2), `fq` is Pallas's (curve 1)."""
import ctypes
import json
import os
import random
import re

import numpy as np
import pytest

import pyref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
_P, _Z, _I, _U32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_uint32
ARGS = {
    # curve, r_f, r_p, out, cap_elems, n_elems
    "h2_poseidon_constants": [_I, _U32, _U32, _P, _Z, ctypes.POINTER(_Z)],
    # curve, r_f, r_p, d_in, d_out, n, stream
    "h2_poseidon_permute_device": [_I, _U32, _U32, _P, _P, _Z, _P],
    # curve, r_f, r_p, d_msgs, len, msg_stride, n, d_out, stream
    "h2_poseidon_hash_device": [_I, _U32, _U32, _P, _Z, _Z, _Z, _P, _P],
    # curve, r_f, r_p, d_leaves, depth, d_nodes, stream
    "h2_poseidon_merkle_device": [_I, _U32, _U32, _P, _U32, _P, _P],
    "h2_poseidon_merkle_tail": [],
    # curve, r_f, r_p, op, in, out
    "h2_selftest_poseidon": [_I, _U32, _U32, _I, _P, _P],
}
FIELD = {0: R.BN_FR, 1: R.PA_FQ, 2: R.PA_FP}
JSON_NAME = {1: "fq", 2: "fp"}
SPEC = {0: (8, 60), 1: (8, 56), 2: (8, 56)}
H2_OK, H2_EINVAL, H2_ENOTINIT = 0, -1, -5
POSEIDON_1_2 = 0x152E960B5C9C8A624B2CDF4855250E8A54EE074254281310DC4A9704F78C1917


def L():
    import halo2_prover_amd
    return halo2_prover_amd.load()


def le(hexstr):
    return int.from_bytes(bytes.fromhex(hexstr), "little")


def vectors():
    return json.load(open(os.path.join(GOLDEN, "pasta_poseidon_vectors.json")))


_REF = {}


def ref_constants(cid, r_f, r_p):
    """pyref's constants, computed once per instance and shared"""
    key = (cid, r_f, r_p)
    if key not in _REF:
        _REF[key] = R.poseidon_constants(FIELD[cid], 3, r_f, r_p)
    return _REF[key]


def limbs(cid, values):
    return np.array([FIELD[cid].limbs(v) for v in values], dtype=np.uint64)


def ints(cid, a):
    raw = np.ascontiguousarray(a, dtype=np.uint64).tobytes()
    return [FIELD[cid].from_mont(int.from_bytes(raw[i:i + 32], "little")) for i in range(0, len(raw), 32)]


def lib_constants(cid, r_f, r_p):
    need = ctypes.c_size_t(0)
    assert L().h2_poseidon_constants(cid, r_f, r_p, None, 0, ctypes.byref(need)) == H2_EINVAL
    assert need.value == 3 * (r_f + r_p) + 9
    out = np.zeros((need.value, 4), dtype=np.uint64)
    assert L().h2_poseidon_constants(cid, r_f, r_p, out.ctypes.data, need.value, ctypes.byref(need)) == H2_OK
    v = ints(cid, out)
    rounds = r_f + r_p
    return [v[3 * r:3 * r + 3] for r in range(rounds)], [v[3 * rounds + 3 * i:3 * rounds + 3 * i + 3] for i in range(3)]


def host_permute(cid, r_f, r_p, state):
    a = limbs(cid, state)
    out = np.zeros((3, 4), dtype=np.uint64)
    assert L().h2_selftest_poseidon(cid, r_f, r_p, 0, a.ctypes.data, out.ctypes.data) == H2_OK
    return ints(cid, out)


def host_hash2(cid, r_f, r_p, msg):
    a = limbs(cid, msg)
    out = np.zeros((1, 4), dtype=np.uint64)
    assert L().h2_selftest_poseidon(cid, r_f, r_p, 1, a.ctypes.data, out.ctypes.data) == H2_OK
    return ints(cid, out)[0]


# ---- the ABI surface --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ARGS))
def test_library_exports_the_entry_point(name):
    assert hasattr(L(), name)
    assert L().h2_version() == 1002


@pytest.mark.parametrize("name", sorted(ARGS))
def test_loader_lists_it_with_its_arguments(name):
    import halo2_prover_amd
    res, args = halo2_prover_amd.SYMBOLS[name]
    assert res is ctypes.c_int and args == ARGS[name]


@pytest.mark.parametrize("name", sorted(ARGS))
def test_a_header_declares_it(name):
    hdr = "h2hip_selftest.h" if name.startswith("h2_selftest_") else "h2hip.h"
    text = open(os.path.join(ROOT, "include", hdr)).read()
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, "include/%s does not declare %s" % (hdr, name)
    params = [] if m.group(1).strip() == "void" else m.group(1).split(",")
    assert len(params) == len(ARGS[name])


def test_the_header_states_the_round_limit_and_the_two_specs():
    text = open(os.path.join(ROOT, "include", "h2hip.h")).read()
    assert int(re.search(r"#define\s+H2_POSEIDON_MAX_ROUNDS\s+(\d+)", text).group(1)) == 128
    assert "P128Pow5T3" in text and "poseidon_circuit.rs" in text


def test_device_calls_fail_loudly_without_a_device():
    """no CPU fallback: H2_ENOTINIT before h2_init (H2_EINVAL's null pointers if a test of this process initialised one)"""
    lib = L()
    assert lib.h2_poseidon_permute_device(1, 8, 56, None, None, 1, None) in (H2_ENOTINIT, H2_EINVAL)
    assert lib.h2_poseidon_hash_device(1, 8, 56, None, 2, 2, 1, None, None) in (H2_ENOTINIT, H2_EINVAL)
    assert lib.h2_poseidon_merkle_device(1, 8, 56, None, 3, None, None) in (H2_ENOTINIT, H2_EINVAL)
    t = lib.h2_poseidon_merkle_tail()
    assert t >= 1 and t & (t - 1) == 0


def test_the_python_layer_exports_the_functions():
    import halo2_prover_amd
    ps = halo2_prover_amd.poseidon
    for name in ("constants", "permute", "hash", "merkle_nodes", "merkle_root", "merkle_path", "verify_path"):
        assert callable(getattr(ps, name)), name


# ---- h2_poseidon_constants --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,r_f,r_p", [(1, 8, 56), (2, 8, 56), (0, 8, 60), (2, 4, 3)])
def test_constants_equal_pyref(cid, r_f, r_p):
    rcs, mds = lib_constants(cid, r_f, r_p)
    want_rcs, want_mds = ref_constants(cid, r_f, r_p)
    assert rcs == want_rcs and mds == want_mds


@pytest.mark.parametrize("cid", [1, 2])
def test_constants_match_the_vectors_spot_values(cid):
    v = vectors()[JSON_NAME[cid]]
    rcs, mds = lib_constants(cid, 8, 56)
    assert "%064x" % rcs[0][0] == v["round_constant_0_0"]
    assert "%064x" % mds[0][0] == v["mds_0_0"]


def test_constants_match_the_recorded_bn256_values():
    rcs, mds = lib_constants(0, 8, 60)
    assert rcs[0][0] == 0x0EE1F344726EBD994115140900A1A52518B73D0D534B720A6CE9B336BDC8F841
    assert mds[0][0] == 0x108C4512F46F539B7732B2A44D80530AE468104492496B33E4162D1C84956E45


def test_constants_python_layer():
    from halo2_prover_amd import poseidon
    rcs, mds = poseidon.constants("pallas", as_int=True)
    assert (rcs, mds) == tuple(ref_constants(1, 8, 56))
    rl, ml = poseidon.constants("bn254")
    assert rl.shape == (68, 3, 4) and ml.shape == (3, 3, 4)


@pytest.mark.parametrize("r_f,r_p", [(7, 56), (0, 56), (2, 127), (128, 2), (130, 0)])
def test_constants_refuse_bad_round_counts(r_f, r_p):
    need = ctypes.c_size_t(0)
    out = np.zeros((3 * 200 + 9, 4), dtype=np.uint64)
    assert L().h2_poseidon_constants(1, r_f, r_p, out.ctypes.data, out.shape[0], ctypes.byref(need)) == H2_EINVAL
    assert not out.any()


def test_constants_refuse_a_short_buffer_and_say_what_is_needed():
    need = ctypes.c_size_t(0)
    out = np.zeros((3 * 64 + 9, 4), dtype=np.uint64)
    assert L().h2_poseidon_constants(1, 8, 56, out.ctypes.data, 3 * 64 + 8, ctypes.byref(need)) == H2_EINVAL
    assert need.value == 3 * 64 + 9 and not out.any()
    assert L().h2_poseidon_constants(9, 8, 56, out.ctypes.data, out.shape[0], ctypes.byref(need)) == H2_EINVAL
    assert L().h2_poseidon_constants(1, 8, 56, out.ctypes.data, out.shape[0], None) == H2_EINVAL
    assert L().h2_poseidon_constants(1, 8, 56, None, out.shape[0], ctypes.byref(need)) == H2_EINVAL
    assert L().h2_poseidon_constants(1, 2, 126, out.ctypes.data, out.shape[0], ctypes.byref(need)) == H2_EINVAL
    assert need.value == 3 * 128 + 9 and not out.any()


# ---- h2_selftest_poseidon: the kernels' template on the host ---------------------------------------------------------
@pytest.mark.parametrize("cid", [1, 2])
def test_host_template_permutes_the_vectors(cid):
    v = vectors()[JSON_NAME[cid]]
    assert len(v["permute"]) == 11
    for t in v["permute"]:
        assert host_permute(cid, 8, 56, [le(x) for x in t["initial_state"]]) == [le(x) for x in t["final_state"]]


@pytest.mark.parametrize("cid", [1, 2])
def test_host_template_hashes_the_vectors(cid):
    v = vectors()[JSON_NAME[cid]]
    assert len(v["hash"]) == 11
    for t in v["hash"]:
        msg = [le(x) for x in t["input"]]
        assert len(msg) == 2
        assert host_hash2(cid, 8, 56, msg) == le(t["output"])


def test_host_template_hashes_one_two_on_bn254():
    assert host_hash2(0, 8, 60, [1, 2]) == POSEIDON_1_2


@pytest.mark.parametrize("cid", [0, 1, 2])
def test_host_template_on_the_extremes_and_random_states(cid):
    """(0, 0, 0) and (p - 1, p - 1, p - 1) are the ends of the bound analysis in csrc/h2_poseidon.hpp"""
    f = FIELD[cid]
    r_f, r_p = SPEC[cid]
    rcs, mds = ref_constants(cid, r_f, r_p)
    rnd = random.Random(0x9051D0 + cid)
    states = [[0, 0, 0], [f.p - 1] * 3, [f.p - 1, 0, 1]] + [[rnd.randrange(f.p) for _ in range(3)] for _ in range(50)]
    for st in states:
        assert host_permute(cid, r_f, r_p, st) == R.poseidon_permute(f, st, rcs, mds, r_f, r_p)
    for st in states[:8]:
        assert host_hash2(cid, r_f, r_p, st[:2]) == R.poseidon_hash_const_len(f, st[:2], rcs, mds, r_f, r_p)


def test_host_template_with_other_round_counts():
    f = FIELD[2]
    rcs, mds = ref_constants(2, 4, 3)
    st = [5, f.p - 1, 1 << 200]
    assert host_permute(2, 4, 3, st) == R.poseidon_permute(f, st, rcs, mds, 4, 3)
    rcs, mds = R.poseidon_constants(f, 3, 2, 0)
    assert host_permute(2, 2, 0, st) == R.poseidon_permute(f, st, rcs, mds, 2, 0)


def test_host_template_refuses_what_it_cannot_run():
    a = np.zeros((3, 4), dtype=np.uint64)
    assert L().h2_selftest_poseidon(1, 7, 56, 0, a.ctypes.data, a.ctypes.data) == H2_EINVAL
    assert L().h2_selftest_poseidon(1, 8, 56, 2, a.ctypes.data, a.ctypes.data) == H2_EINVAL
    assert L().h2_selftest_poseidon(5, 8, 56, 0, a.ctypes.data, a.ctypes.data) == H2_EINVAL
    assert L().h2_selftest_poseidon(1, 8, 56, 0, None, a.ctypes.data) == H2_EINVAL


# ---- the Python host helpers -----------------------------------------------------------------------------------------
def test_merkle_path_and_verify_path_round_trip():
    from halo2_prover_amd import poseidon
    cid, depth = 1, 3
    f = FIELD[cid]
    rcs, mds = ref_constants(cid, 8, 56)
    rnd = random.Random(77)
    level = [rnd.randrange(f.p) for _ in range(1 << depth)]
    tree = list(level)
    while len(level) > 1:
        level = [R.poseidon_hash_const_len(f, level[2 * i:2 * i + 2], rcs, mds, 8, 56) for i in range(len(level) // 2)]
        tree += level
    root = tree[-1]
    assert len(tree) == (2 << depth) - 1
    for index in range(1 << depth):
        path = poseidon.merkle_path(tree, depth, index)
        assert len(path) == depth
        assert poseidon.verify_path(cid, tree[index], index, path, root)
        assert not poseidon.verify_path(cid, (tree[index] + 1) % f.p, index, path, root)
        assert not poseidon.verify_path(cid, tree[index], index ^ 1, path, root)
        bad = list(path)
        bad[1] = (bad[1] + 1) % f.p
        assert not poseidon.verify_path(cid, tree[index], index, bad, root)
    with pytest.raises(ValueError):
        poseidon.merkle_path(tree[:-1], depth, 0)
    with pytest.raises(ValueError):
        poseidon.merkle_path(tree, depth, 1 << depth)
