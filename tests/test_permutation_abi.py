"""CPU (no GPU): the ABI of h2_permutation_product_device / h2_permutation_tile -- exported by the built library, listed by
the Python loader with their argument lists, declared in include/h2hip.h; h2_version() did not move (a host detects the
entry points by their symbols); the tile size is known without a device."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_P, _Z, _I = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
ARGS = {
    # curve, d_values, d_sigma, n_cols, chunk_len, usable_rows, m, beta, gamma, omega, delta, d_z, col_stride, stream
    "h2_permutation_product_device": [_I, _P, _P, _Z, _Z, _Z, _Z, _P, _P, _P, _P, _P, _Z, _P],
    "h2_permutation_tile": [],
}


@pytest.mark.parametrize("name", sorted(ARGS))
def test_library_exports_the_entry_point(name):
    import halo2_prover_amd
    lib = halo2_prover_amd.load()
    assert hasattr(lib, name)
    assert lib.h2_version() == 1002


@pytest.mark.parametrize("name", sorted(ARGS))
def test_loader_lists_it_with_its_arguments(name):
    import halo2_prover_amd
    res, args = halo2_prover_amd.SYMBOLS[name]
    assert res is ctypes.c_int and args == ARGS[name]


@pytest.mark.parametrize("name", sorted(ARGS))
def test_header_declares_it(name):
    text = open(os.path.join(ROOT, "include", "h2hip.h")).read()
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, "include/h2hip.h does not declare " + name
    params = m.group(1).strip()
    count = 0 if params == "void" else len(params.split(","))
    assert count == len(ARGS[name])


def test_tile_is_a_power_of_two_without_init():
    import halo2_prover_amd
    T = halo2_prover_amd.load().h2_permutation_tile()
    assert T >= 64 and T & (T - 1) == 0


def test_it_fails_loudly_without_init():
    """no CPU fallback: before h2_init the call is H2_ENOTINIT (H2_EINVAL's null pointers if another test of this process
    has initialised a device)"""
    import halo2_prover_amd
    lib = halo2_prover_amd.load()
    c = (ctypes.c_uint64 * 4)(1, 0, 0, 0)
    assert lib.h2_permutation_product_device(0, None, None, 3, 2, 8, 1, c, c, c, c, None, 9, None) in (-5, -1)


def test_the_python_layer_exports_it():
    import halo2_prover_amd
    assert callable(halo2_prover_amd.permutation_product)
