"""CPU (no GPU): the ABI of h2_poseidon_merkle_{paths,verify,update}_device and of the hook that fixes the walker's form --
exported, listed by the loader with their arguments, declared in the headers, the status words #defined, h2_version()
unmoved, and H2_ENOTINIT before h2_init (there is no CPU fallback)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_P, _Z, _I, _U32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_uint32
ARGS = {
    # curve, d_leaves, d_nodes, depth, d_indices, n, d_paths, d_status, stream
    "h2_poseidon_merkle_paths_device": [_I, _P, _P, _U32, _P, _Z, _P, _P, _P],
    # curve, r_f, r_p, d_leaf_values, d_indices, d_paths, depth, n, d_root, d_roots_out, d_status, stream
    "h2_poseidon_merkle_verify_device": [_I, _U32, _U32, _P, _P, _P, _U32, _Z, _P, _P, _P, _P],
    # curve, r_f, r_p, d_leaves, d_nodes, depth, d_indices, d_values, n, d_status, stream
    "h2_poseidon_merkle_update_device": [_I, _U32, _U32, _P, _P, _U32, _P, _P, _Z, _P, _P],
    "h2_selftest_set_poseidon_walk_form": [_I],
}
STATUS = {"H2_MERKLE_OK": 0, "H2_MERKLE_RANGE": 1, "H2_MERKLE_NONCANONICAL": 2, "H2_MERKLE_SUPERSEDED": 3, "H2_MERKLE_MISMATCH": 4}
H2_OK, H2_EINVAL, H2_ENOTINIT = 0, -1, -5


def L():
    import halo2_prover_amd
    return halo2_prover_amd.load()


@pytest.mark.parametrize("name", sorted(ARGS))
def test_library_exports_the_entry_point(name):
    assert hasattr(L(), name)
    assert L().h2_version() == 1002


@pytest.mark.parametrize("name", sorted(ARGS))
def test_loader_lists_it_with_its_arguments(name):
    from halo2_prover_amd import lib
    res, args = (lib.SELFTEST_SYMBOLS if name.startswith("h2_selftest_") else lib.SYMBOLS)[name]
    assert res is ctypes.c_int and args == ARGS[name]


@pytest.mark.parametrize("name", sorted(ARGS))
def test_a_header_declares_it(name):
    hdr = "h2hip_selftest.h" if name.startswith("h2_selftest_") else "h2hip.h"
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", hdr)).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, "include/%s does not declare %s" % (hdr, name)
    assert len(m.group(1).split(",")) == len(ARGS[name])


@pytest.mark.parametrize("name", sorted(STATUS))
def test_the_header_defines_the_status_word(name):
    text = open(os.path.join(ROOT, "include", "h2hip.h")).read()
    m = re.search(r"#define\s+" + name + r"\s+(\d+)", text)
    assert m and int(m.group(1)) == STATUS[name]


def test_the_python_layer_knows_the_same_status_words_and_exports_the_functions():
    import halo2_prover_amd
    ps = halo2_prover_amd.poseidon
    assert (ps.STATUS_OK, ps.STATUS_RANGE, ps.STATUS_NONCANONICAL, ps.STATUS_SUPERSEDED, ps.STATUS_MISMATCH) == (0, 1, 2, 3, 4)
    for name in ("merkle_paths", "verify_paths", "merkle_update", "merkle_path", "verify_path"):
        assert callable(getattr(ps, name)), name


def test_device_calls_fail_loudly_without_a_device():
    """H2_ENOTINIT before h2_init (H2_EINVAL's null pointers if a test of this process initialised a device)"""
    lib = L()
    assert lib.h2_poseidon_merkle_paths_device(1, None, None, 3, None, 1, None, None, None) in (H2_ENOTINIT, H2_EINVAL)
    assert lib.h2_poseidon_merkle_verify_device(1, 8, 56, None, None, None, 3, 1, None, None, None, None) in (H2_ENOTINIT, H2_EINVAL)
    assert lib.h2_poseidon_merkle_update_device(1, 8, 56, None, None, 3, None, None, 1, None, None) in (H2_ENOTINIT, H2_EINVAL)


def test_the_walk_form_hook_takes_its_three_values_and_no_other():
    lib = L()
    try:
        for form in (1, 2, 0):
            assert lib.h2_selftest_set_poseidon_walk_form(form) == H2_OK
        assert lib.h2_selftest_set_poseidon_walk_form(3) == H2_EINVAL
        assert lib.h2_selftest_set_poseidon_walk_form(-1) == H2_EINVAL
    finally:
        assert lib.h2_selftest_set_poseidon_walk_form(0) == H2_OK
