"""A cached proving key must outlive the list that shares its domain tables.

The C++ prover keeps, per domain shape (k, extended k, blinding rows), the device columns every key of that shape uses
(w^i, X and the Lagrange combinations on the extended coset, 1 / (X^n - 1)) in a list of eight, oldest dropped first,
and keeps the last six keys.  A key that is still cached when its shape leaves the list has to keep those columns
alive: otherwise the next proof made with it reads buffers that were handed to somebody else.  A long-lived process that
serves more than eight shapes gets there, and so does the test suite.
"""
import pytest

from test_capi_product import c_prove, c_setup, c_verify

pytestmark = pytest.mark.gpu
SHAPES = (5, 9, 12, 13, 14, 15, 17, 18)          # k of the arithmetic circuit: sizes no other test uses
ONE_MORE = 19


@pytest.fixture(scope="module")
def lib():
    import halo2_prover_amd
    return halo2_prover_amd.load()


def test_a_cached_key_survives_the_turnover_of_the_domain_tables(h2, lib):
    js = '{"x":3,"y":5,"constant":11,"z":%d}' % (3 * 3 * 5 * 5 + 11)
    params = {k: c_setup(lib, k, None) for k in SHAPES}
    old = lib.h2_key_cache(0)
    try:
        for k in SHAPES:                           # eight new shapes, keys not kept: SHAPES[0] is now the oldest of the list
            assert c_verify(lib, params[k], c_prove(lib, params[k], js, 1, None), js, 1) == (0, 1), k
        lib.h2_key_cache(1)
        first = params[SHAPES[0]]
        assert c_verify(lib, first, c_prove(lib, first, js, 1, None), js, 1) == (0, 1)      # its key is cached now
        last = c_setup(lib, ONE_MORE, None)        # a ninth shape: the oldest one leaves the list
        assert c_verify(lib, last, c_prove(lib, last, js, 1, None), js, 1) == (0, 1)
        for _ in range(3):                         # the cached key still proves
            assert c_verify(lib, first, c_prove(lib, first, js, 1, None), js, 1) == (0, 1)
    finally:
        lib.h2_key_cache(old)
        lib.h2_params_cache_clear()
