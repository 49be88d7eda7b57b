"""CPU (no GPU): the ABI of the lockstep inner product argument, h2_ipa_*_batch_device -- exported by the built library,
listed by the Python loader with their argument lists, declared in include/h2hip.h with the same arity; H2_IPA_MAX_BATCH is
defined; h2_version() did not move; the batch state's size is known without a device and bounded from below by what m
openings and their 2 m columns take."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_P, _Z, _I, _U32, _U64 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint64
ARGS = {
    # k, m, out
    "h2_ipa_batch_state_bytes": [_U32, _Z, ctypes.POINTER(_Z)],
    # curve, k, m, d_p, x3, d_state, stream
    "h2_ipa_begin_batch_device": [_I, _U32, _Z, _P, _P, _P, _P],
    # curve, bases, k, j, m, d_state, u_prev, u_prev_inv, z, l_blind, r_blind, d_out_affine, stream
    "h2_ipa_round_batch_device": [_I, _U64, _U32, _U32, _Z, _P, _P, _P, _P, _P, _P, _P, _P],
    # curve, k, m, d_state, u_last, u_last_inv, d_out, stream
    "h2_ipa_final_batch_device": [_I, _U32, _Z, _P, _P, _P, _P, _P],
}
H2_EINVAL = -1


def header():
    return open(os.path.join(ROOT, "include", "h2hip.h")).read()


def define(name):
    m = re.search(r"#define\s+" + name + r"\s+(\d+)", header())
    assert m, "include/h2hip.h does not define " + name
    return int(m.group(1))


@pytest.mark.parametrize("name", sorted(ARGS))
def test_library_exports_the_entry_point(name):
    import halo2_prover_amd
    lib = halo2_prover_amd.load()
    assert hasattr(lib, name)
    assert lib.h2_version() == 1002


@pytest.mark.parametrize("name", sorted(ARGS))
def test_loader_lists_it_with_its_arguments(name):
    import halo2_prover_amd
    assert name in halo2_prover_amd.SYMBOLS, "lib.py's SYMBOLS does not list " + name
    res, args = halo2_prover_amd.SYMBOLS[name]
    assert res is ctypes.c_int and args == ARGS[name]


@pytest.mark.parametrize("name", sorted(ARGS))
def test_header_declares_it(name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header())
    assert m, "include/h2hip.h does not declare " + name
    assert len(m.group(1).split(",")) == len(ARGS[name])


def test_the_header_states_the_largest_batch():
    assert define("H2_IPA_MAX_BATCH") == 64
    from halo2_prover_amd import ipa
    assert ipa.MAX_BATCH == 64 and callable(ipa.create_proofs)


def test_batch_state_bytes_without_init():
    """host only: a multiple of 16, at least m (4 n + 2 (n + 2)) elements of 32 bytes (a, b in two generations, s, two
    columns of n + 2 per opening), strictly increasing in m and in k"""
    import halo2_prover_amd
    lib = halo2_prover_amd.load()
    max_k, max_m = define("H2_IPA_MAX_K"), define("H2_IPA_MAX_BATCH")
    out = ctypes.c_size_t(0)
    size = {}
    for k in range(1, max_k + 1):
        n = 1 << k
        for m in (1, 2, 3, 5, 26, max_m - 1, max_m):
            assert lib.h2_ipa_batch_state_bytes(k, m, ctypes.byref(out)) == 0
            assert out.value % 16 == 0
            assert out.value >= m * (4 * n + 2 * (n + 2)) * 32
            size[k, m] = out.value
    for k in (1, 4, max_k):                                     # every m at a few k
        row = []
        for m in range(1, max_m + 1):
            assert lib.h2_ipa_batch_state_bytes(k, m, ctypes.byref(out)) == 0
            row.append(out.value)
        assert all(a < b for a, b in zip(row, row[1:]))
    for m in (1, 5, max_m):
        col = [size[k, m] for k in range(1, max_k + 1)]
        assert all(a < b for a, b in zip(col, col[1:]))


def test_batch_state_bytes_refuses_the_ends():
    import halo2_prover_amd
    lib = halo2_prover_amd.load()
    max_k, max_m = define("H2_IPA_MAX_K"), define("H2_IPA_MAX_BATCH")
    out = ctypes.c_size_t(0)
    assert lib.h2_ipa_batch_state_bytes(0, 1, ctypes.byref(out)) == H2_EINVAL
    assert lib.h2_ipa_batch_state_bytes(max_k + 1, 1, ctypes.byref(out)) == H2_EINVAL
    assert lib.h2_ipa_batch_state_bytes(4, 0, ctypes.byref(out)) == H2_EINVAL
    assert lib.h2_ipa_batch_state_bytes(4, max_m + 1, ctypes.byref(out)) == H2_EINVAL
    assert lib.h2_ipa_batch_state_bytes(4, 3, None) == H2_EINVAL
    assert lib.h2_ipa_batch_state_bytes(max_k, max_m, ctypes.byref(out)) == 0


def test_they_fail_loudly_without_init():
    """no CPU fallback: before h2_init the calls are H2_ENOTINIT (H2_EINVAL's null pointers if another test of this
    process has initialised a device)"""
    import halo2_prover_amd
    lib = halo2_prover_amd.load()
    c = (ctypes.c_uint64 * 4)(1, 0, 0, 0)
    ptrs = (ctypes.c_void_p * 1)(None)
    assert lib.h2_ipa_begin_batch_device(1, 4, 1, ptrs, c, None, None) in (-5, -1)
    assert lib.h2_ipa_round_batch_device(1, 1, 4, 0, 1, None, None, None, c, c, c, None, None) in (-5, -1)
    assert lib.h2_ipa_final_batch_device(1, 4, 1, None, c, c, None, None) in (-5, -1)
