"""CPU (no GPU): the ABI of h2_poly_lincomb_device / h2_poly_lincomb_max_rounds -- exported by the built library, listed by
the Python loader with their argument lists, declared in include/h2hip.h; h2_version() did not move (a host detects the
entry points by their symbols); the two table structs have the C layout; the round limit is known without a device."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_P, _Z, _I = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
ARGS = {
    # curve, jobs, n_jobs, terms, n_terms, low, n_low, points, n_points, n, stream
    "h2_poly_lincomb_device": [_I, _P, _Z, _P, _Z, _P, _Z, _P, _Z, _Z, _P],
    "h2_poly_lincomb_max_rounds": [],
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


def test_the_header_says_the_version_stays():
    text = open(os.path.join(ROOT, "include", "h2hip.h")).read()
    at = text.index("h2_lincomb_term_t")
    assert "1002" in text[text.rindex("/*", 0, at):at]


def test_the_mirrored_structs_have_the_c_layout():
    from halo2_prover_amd import opening
    assert ctypes.sizeof(opening.LincombTerm) == 40
    assert ctypes.sizeof(opening.LincombJob) == 32
    assert opening.LincombTerm.coeff.offset == 8
    assert [getattr(opening.LincombJob, f).offset for f in
            ("d_out", "first_term", "n_terms", "first_low", "n_low", "first_point", "n_points")] == [0, 8, 12, 16, 20, 24, 28]


def test_max_rounds_needs_no_init():
    import halo2_prover_amd
    assert halo2_prover_amd.load().h2_poly_lincomb_max_rounds() >= 3


def test_it_fails_loudly_without_init():
    """no CPU fallback: before h2_init the call is H2_ENOTINIT (H2_EINVAL's null pointers if another test of this process
    has initialised a device)"""
    import halo2_prover_amd
    from halo2_prover_amd import opening
    lib = halo2_prover_amd.load()
    job = (opening.LincombJob * 1)()
    job[0].n_terms = 1
    assert lib.h2_poly_lincomb_device(0, job, 1, None, 0, None, 0, None, 0, 16, None) in (-5, -1)


@pytest.mark.parametrize("name", ["poly_lincomb", "gwc_open", "shplonk_open_h", "shplonk_open_final"])
def test_the_python_layer_exports_it(name):
    import halo2_prover_amd
    assert callable(getattr(halo2_prover_amd, name))
