"""CPU (no GPU): the ABI of the IPA prover behind one call -- h2_ipa_prove_state_bytes, h2_ipa_prove_rounds_device and
h2_ipa_create_proofs are exported by the built library, listed by the Python loader with their argument lists and declared
in include/h2hip.h with the same arity; h2_version() did not move; the prove state's size is known without a device, holds
the batch state in front and grows with m and with k; ipa.create_proofs_bytes is there."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_P, _Z, _I, _U32, _U64 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint64
ARGS = {
    # k, m, out
    "h2_ipa_prove_state_bytes": [_U32, _Z, ctypes.POINTER(_Z)],
    # curve, bases, k, m, d_p, x3, z, f0, round_blinds, states, d_state, d_tail, d_states_out, d_status, stream
    "h2_ipa_prove_rounds_device": [_I, _U64, _U32, _Z, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P],
    # curve, bases, k, m, states, d_p, p_blind, x3, d_s_poly, seeds, s_blind, round_blinds, proofs, states_out, status
    "h2_ipa_create_proofs": [_I, _U64, _U32, _Z, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P],
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


def test_the_python_route_is_there():
    from halo2_prover_amd import ipa
    assert callable(ipa.create_proofs_bytes) and callable(ipa.create_proofs)


def test_prove_state_bytes_without_init():
    """host only: a multiple of 16, at least the batch state plus 2 k blinds, f, a midstate and a round's two points per
    opening, strictly increasing in m and in k"""
    import halo2_prover_amd
    lib = halo2_prover_amd.load()
    max_k, max_m = define("H2_IPA_MAX_K"), define("H2_IPA_MAX_BATCH")
    out, inner = ctypes.c_size_t(0), ctypes.c_size_t(0)
    size = {}
    for k in range(1, max_k + 1):
        for m in (1, 2, 3, 5, 26, max_m - 1, max_m):
            assert lib.h2_ipa_prove_state_bytes(k, m, ctypes.byref(out)) == 0
            assert lib.h2_ipa_batch_state_bytes(k, m, ctypes.byref(inner)) == 0
            assert out.value % 16 == 0
            assert out.value >= inner.value + m * (2 * k * 32 + 32 + 208 + 128)
            size[k, m] = out.value
    for k in (1, 4, max_k):                                     # every m at a few k
        row = []
        for m in range(1, max_m + 1):
            assert lib.h2_ipa_prove_state_bytes(k, m, ctypes.byref(out)) == 0
            row.append(out.value)
        assert all(a < b for a, b in zip(row, row[1:]))
    for m in (1, 5, max_m):
        col = [size[k, m] for k in range(1, max_k + 1)]
        assert all(a < b for a, b in zip(col, col[1:]))


def test_prove_state_bytes_refuses_the_ends():
    import halo2_prover_amd
    lib = halo2_prover_amd.load()
    max_k, max_m = define("H2_IPA_MAX_K"), define("H2_IPA_MAX_BATCH")
    out = ctypes.c_size_t(0)
    assert lib.h2_ipa_prove_state_bytes(0, 1, ctypes.byref(out)) == H2_EINVAL
    assert lib.h2_ipa_prove_state_bytes(max_k + 1, 1, ctypes.byref(out)) == H2_EINVAL
    assert lib.h2_ipa_prove_state_bytes(4, 0, ctypes.byref(out)) == H2_EINVAL
    assert lib.h2_ipa_prove_state_bytes(4, max_m + 1, ctypes.byref(out)) == H2_EINVAL
    assert lib.h2_ipa_prove_state_bytes(4, 3, None) == H2_EINVAL
    assert lib.h2_ipa_prove_state_bytes(max_k, max_m, ctypes.byref(out)) == 0


def test_they_fail_loudly_without_init():
    """no CPU fallback: before h2_init the calls are H2_ENOTINIT (H2_EINVAL's null pointers if another test of this
    process has initialised a device)"""
    import halo2_prover_amd
    lib = halo2_prover_amd.load()
    c = (ctypes.c_uint64 * 8)(1, 0, 0, 0, 1, 0, 0, 0)
    ptrs = (ctypes.c_void_p * 1)(None)
    state = ctypes.create_string_buffer(208)
    assert lib.h2_ipa_prove_rounds_device(1, 1, 1, 1, ptrs, c, c, c, c, state, None, None, None, None, None) in (-5, -1)
    assert lib.h2_ipa_create_proofs(1, 1, 1, 1, state, ptrs, c, c, ptrs, None, c, c, None, None, None) in (-5, -1)
