"""The working-form group law of h2_curve29.hpp (xyzz29_add, xyzz29_double, xyzz29_add_affine, xyzz29_double_affine) on
raw operands over the WHOLE stored range of every coordinate -- x in (-3p, 5p), y in (-2p, 2p), zz and zzz in (-3p/2, p),
affine y as loaded or limb-wise negated -- through the host instantiation (h2_selftest_xyzz29_op; no GPU).

For every case of oracle/xyzz29_cases.py:
* the 36 output limbs equal pyref's limb-exact model (same operation order as the HIP source);
* independently of the model, by big integers only: the output is a stored point inside the contract (limbs normalised,
  each coordinate strictly inside its range; the one-lane forms return y in (-3p/2, p/2]) and stands for Curve.add of
  the affine points; the identity is judged by zz exactly zero and nothing else of it is used;
* the model's checking mode raised nothing: every product within its limb bounds and 64 p^2, every zero test below 16 p.
The case lists are classified with big integers (generic, doubling, cancelling, identity-in) and every class that
applies to an op has to be populated; the Q = +-P sweeps have to reach every multiple of p the ranges allow at the zero
tests.  tests/test_gpu_xyzz29_ranges.py runs the same cases through the device instantiation."""
import ctypes

import numpy as np
import pytest

import pyref as R
import xyzz29_cases as X

HOST_OPS = (X.ADD, X.DOUBLE, X.ADD_AFFINE, X.DOUBLE_AFFINE)
ONE_LANE_Y2 = (-3, 1)          # (-3p/2, p/2] in units of p / 2 (p is odd: the closed end is never met)


@pytest.fixture(scope="module")
def lib():
    import halo2_prover_amd
    return halo2_prover_amd.load()


@pytest.mark.parametrize("op", HOST_OPS)
@pytest.mark.parametrize("name", list(R.CURVES))
def test_host_group_law_over_the_stored_ranges(lib, name, op):
    curve = R.CURVES[name]
    cs = X.cases_of(name, op)
    counts = X.class_counts(name, op)
    assert all(counts.values()), counts                    # a case list that stops covering a branch fails here
    want, chk = X.modelled(name, op)                       # raises if the model's own preconditions break
    got = X.host_rows(lib, curve.cid, op, [c.row for c in cs])
    for i, c in enumerate(cs):
        out = [int(v) for v in got[i]]
        cls = X.classify(curve, op, c.P, c.Q)
        assert out == want[i], (name, op, i, cls)
        # an operand handed back unchanged (identity-in) keeps its own y; a computed y is one product's result
        y2 = X.RANGE2["y"] if cls == "identity-in" else ONE_LANE_Y2
        err = X.check_result(curve, out, X.expected(curve, op, c.P, c.Q), y2)
        assert err is None, (name, op, i, cls, err)
    assert chk.max_product <= 64 and chk.max_zero_test < 16
    print("%s op %d: %d cases %s; largest product %.1f p^2, largest zero test %.2f p"
          % (name, op, len(cs), counts, chk.max_product, chk.max_zero_test))


@pytest.mark.parametrize("name", list(R.CURVES))
def test_the_sweeps_reach_every_multiple_of_p_at_the_zero_tests(name):
    """from the model: u2 - acc.x of xyzz29_add_affine ran through j p for j = -5..3 (acc.x over its eight
    representatives against a product in (-p, 0]), and xyzz29_add's p and r met both signs and zero"""
    seen = {}
    for op in (X.ADD, X.ADD_AFFINE):
        seen.update(X.modelled(name, op)[1].zero_multiples)
    assert seen["add_affine.p"] >= set(range(-5, 4)), seen
    assert {j for j in seen["add_affine.r"] if j} and 0 in seen["add_affine.r"], seen
    for k in ("add.p", "add.r"):
        assert 0 in seen[k] and min(seen[k]) < 0 < max(seen[k]), seen


def test_the_hook_refuses_what_it_does_not_have(lib):
    row = np.zeros(72, dtype=np.int32)
    out = np.full(36, 7, dtype=np.int32)
    for curve, op in ((3, 0), (-1, 0), (0, 4), (0, -1)):
        assert lib.h2_selftest_xyzz29_op(curve, op, row.ctypes.data, out.ctypes.data) != 0
    assert lib.h2_selftest_xyzz29_op(0, 0, None, out.ctypes.data) != 0
    assert (out == 7).all()
