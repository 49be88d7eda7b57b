"""The cases of tests/test_xyzz29_ranges.py (oracle/xyzz29_cases.py: every stored coordinate anywhere in its range)
through the DEVICE instantiation of the working-form group law, h2_selftest_xyzz29_op_device: one launch per op, four
lanes per operand pair, every lane's copy of the result read back.

* ops 0..3 (xyzz29_add, xyzz29_double, xyzz29_add_affine, xyzz29_double_affine): the host hook's limbs;
* ops 4, 5 (xyzz29_add_quad, xyzz29_double_quad): the limbs of pyref's quad model, and the four lanes' copies identical;
* ops 6, 7 (the affine forms on Fe29Chain, the accumulate kernel's instantiation): the limbs of ops 2, 3 on Pallas and
  Vesta; H2_EINVAL and nothing written on BN254;
* every result a stored point inside the contract that stands for Curve.add of the operands, by big integers only
  (xyzz29_add_quad's y anywhere in (-2p, 2p), the one-lane forms' in (-3p/2, p/2]);
* a chain per op: a result at the edge of x's range fed back as operand A 64 times against fresh operands B, the
  model followed in step -- the induction the MSM's accumulators rely on."""
import random

import numpy as np
import pytest

import pyref as R
import xyzz29_cases as X

pytestmark = pytest.mark.gpu

H2_EINVAL = -1
ONE_LANE_Y2 = (-3, 1)          # (-3p/2, p/2] in units of p / 2
CHAINED = {"bn254": (), "pallas": (X.ADD_AFFINE_CHAIN, X.DOUBLE_AFFINE_CHAIN), "vesta": (X.ADD_AFFINE_CHAIN, X.DOUBLE_AFFINE_CHAIN)}


def replicated(out):
    """(n, 4, 36): the four lanes' copies are identical -> lane 0's, as lists of ints"""
    assert (out == out[:, :1, :]).all(), np.argwhere((out != out[:, :1, :]).any(axis=(1, 2)))[:8]
    return out[:, 0, :].tolist()


def check_points(curve, name, op, got):
    cs = X.cases_of(name, op)
    counts = X.class_counts(name, op)
    assert all(counts.values()), counts
    quad = op in (X.ADD_QUAD, X.DOUBLE_QUAD)
    for i, c in enumerate(cs):
        cls = X.classify(curve, op, c.P, c.Q)
        y2 = X.RANGE2["y"] if quad or cls == "identity-in" else ONE_LANE_Y2
        err = X.check_result(curve, got[i], X.expected(curve, op, c.P, c.Q), y2)
        assert err is None, (name, op, i, cls, err)


@pytest.mark.parametrize("op", (X.ADD, X.DOUBLE, X.ADD_AFFINE, X.DOUBLE_AFFINE))
@pytest.mark.parametrize("name", list(R.CURVES))
def test_device_one_lane_forms_give_the_host_limbs(h2, name, op):
    lib, curve = h2.load(), R.CURVES[name]
    rows = [c.row for c in X.cases_of(name, op)]
    got = replicated(X.device_rows(lib, curve.cid, op, rows))
    host = X.host_rows(lib, curve.cid, op, rows).tolist()
    for i in range(len(rows)):
        assert got[i] == host[i], (name, op, i)
    check_points(curve, name, op, got)


@pytest.mark.parametrize("op", (X.ADD_QUAD, X.DOUBLE_QUAD))
@pytest.mark.parametrize("name", list(R.CURVES))
def test_device_quad_forms_give_the_model_limbs_in_every_lane(h2, name, op):
    lib, curve = h2.load(), R.CURVES[name]
    want, chk = X.modelled(name, op)                       # raises if the quad model's own preconditions break
    got = replicated(X.device_rows(lib, curve.cid, op, [c.row for c in X.cases_of(name, op)]))
    for i in range(len(want)):
        assert got[i] == want[i], (name, op, i)
    check_points(curve, name, op, got)
    assert chk.max_product <= 64 and chk.max_zero_test < 16
    print("%s op %d: largest product %.1f p^2, largest zero test %.2f p" % (name, op, chk.max_product, chk.max_zero_test))


@pytest.mark.parametrize("op", (X.ADD_AFFINE_CHAIN, X.DOUBLE_AFFINE_CHAIN))
@pytest.mark.parametrize("name", ("pallas", "vesta"))
def test_device_chain_forms_give_the_compiler_forms_limbs(h2, name, op):
    lib, curve = h2.load(), R.CURVES[name]
    rows = [c.row for c in X.cases_of(name, op)]
    got = replicated(X.device_rows(lib, curve.cid, op, rows))
    plain = replicated(X.device_rows(lib, curve.cid, op - 4, rows))
    host = X.host_rows(lib, curve.cid, op - 4, rows).tolist()
    for i in range(len(rows)):
        assert got[i] == plain[i] == host[i], (name, op, i)
    check_points(curve, name, op, got)


@pytest.mark.parametrize("op", (X.ADD_AFFINE_CHAIN, X.DOUBLE_AFFINE_CHAIN))
def test_bn254_has_no_chain_form(h2, op):
    lib = h2.load()
    rows = np.array([c.row for c in X.cases_of("bn254", op)[:4]], dtype=np.int64).astype(np.int32)
    out = np.full((4, 4, 36), 7, dtype=np.int32)
    assert lib.h2_selftest_xyzz29_op_device(0, op, rows.ctypes.data, out.ctypes.data, 4) == H2_EINVAL
    assert (out == 7).all()
    for curve, bad_op, n in ((0, 8, 4), (0, -1, 4), (3, 0, 4), (0, 0, 0), (0, 0, (1 << 20) + 1)):
        assert lib.h2_selftest_xyzz29_op_device(curve, bad_op, rows.ctypes.data, out.ctypes.data, n) == H2_EINVAL
    assert (out == 7).all()


@pytest.mark.parametrize("name", list(R.CURVES))
def test_results_at_the_range_edge_chain_64_times(h2, name):
    """operand A of step i + 1 is the device's own result of step i, starting from the results of the generic additions
    with the lowest and the highest x; B is fresh every step (affine: as loaded and negated in turn)"""
    lib, curve = h2.load(), R.CURVES[name]
    p = curve.base.p
    cs, (outs, _) = X.cases_of(name, X.ADD), X.modelled(name, X.ADD)
    generic = [i for i, c in enumerate(cs) if X.classify(curve, X.ADD, c.P, c.Q) == "generic"]
    xs = {i: R.fe29_value(outs[i][:9]) for i in generic}
    starts = [min(generic, key=xs.get), max(generic, key=xs.get)]
    # x3 = rr - ppp - 2 qq with every product in (-p, 0] up to a b / R': a computed x lies in about (-p, 3p), inside
    # the (-3p, 5p) the contract grants; the starts are within p / 2 of either end of what is reached
    assert 2 * xs[starts[0]] < -p and 2 * xs[starts[1]] > 5 * p, [xs[i] / p for i in starts]
    for op in (X.ADD, X.DOUBLE, X.ADD_AFFINE, X.ADD_QUAD, X.DOUBLE_QUAD) + CHAINED[name][:1]:
        rng = random.Random(1000 * curve.cid + op)
        acc = [list(outs[i]) for i in starts]
        pts = [curve.add(cs[i].P, cs[i].Q) for i in starts]
        quad = op in (X.ADD_QUAD, X.DOUBLE_QUAD)
        walk, stride = (curve.mul(rng.randrange(1, curve.scalar.p), curve.gen) for _ in range(2))   # fresh B's: walk + i stride
        for step in range(64):
            rows, fresh = [], []
            for a in acc:
                Q = walk = curve.add(walk, stride)
                fresh.append(Q)
                if op in X.PROJECTIVE_OPS:
                    mu = rng.choice((1, rng.randrange(2, p)))
                    hows = tuple(rng.choice(("lo", "hi", "rand")) for _ in range(2)) + \
                        ((0, 0) if mu == 1 else tuple(rng.choice(("lo", "hi", "rand")) for _ in range(2)))
                    rows.append(a + X.stored(curve, Q, mu, hows, rng))
                else:
                    rows.append(a + X.table_entry(curve, Q, bool(step & 1)) + [0] * 18)
            got = replicated(X.device_rows(lib, curve.cid, op, rows))
            for k in range(len(acc)):
                assert got[k] == X.model_row(name, op, rows[k], R.Fe29Check(p)), (name, op, step, k)
                pts[k] = X.expected(curve, op, pts[k], fresh[k])
                err = X.check_result(curve, got[k], pts[k], X.RANGE2["y"] if quad else ONE_LANE_Y2)
                assert err is None, (name, op, step, k, err)
                acc[k] = got[k]
