"""The four-lanes-per-point addition and doubling (csrc/h2_curve_quad.hpp, routed operands) on the device, 64 operand
pairs a curve, by two doors:

* h2_selftest_curve_op_device (affine points in the API form in and out): quad add (op 0), quad double (1) and the
  addition behind a doubling (4) against big integers;
* h2_selftest_xyzz29_op_device (stored operands, raw limbs in and out): the same three on stored points whose
  coordinates sit at the low end, the high end and inside their ranges, every lane's copy of the result read back: the
  four copies identical, the 36 words inside the CLOSURE ranges of h2_curve29.hpp, the point the expected one, and the
  limbs those of pyref's model of the quad forms (which multiplies the operands the first version of the header
  multiplied: the routed form must give the same integers).

The pairs: random points, P + P, P - P, O + Q, P + O, O + O, and the identity that a P - P on the device returned as
an operand of the next addition (no point of these curves has y = 0, so that is the one way to an identity).
There is one product form for the quad operations (the compiler's), so there is no second policy to compare with."""
import random

import numpy as np
import pytest

import pyref as R
import xyzz29_cases as X

pytestmark = pytest.mark.gpu

N = 64
HOWS = ("lo", "hi", "rand")


def pairs(curve):
    rng = random.Random(0x51AD0 + curve.cid)
    order = curve.scalar.p
    Ps = [curve.mul(rng.randrange(1, order), curve.gen) for _ in range(N)]
    Qs = [curve.mul(rng.randrange(1, order), curve.gen) for _ in range(N)]
    for i in range(0, 8):
        Qs[i] = Ps[i]                       # P + P
    for i in range(8, 16):
        Qs[i] = curve.neg(Ps[i])            # P - P
    for i in range(16, 20):
        Ps[i] = None                        # O + Q
    for i in range(20, 24):
        Qs[i] = None                        # P + O
    Ps[24] = Qs[24] = Ps[25] = Qs[25] = None
    return Ps, Qs, rng


def stored_rows(curve, Ps, Qs, rng):
    """every pair as two stored points: the first 3 x 3 x ... pairs walk the ends of the ranges coordinate by
    coordinate, the others draw a representative per coordinate"""
    p = curve.base.p
    rows = []
    for i, (P, Q) in enumerate(zip(Ps, Qs)):
        lam, mu = rng.randrange(2, p), rng.choice((1, rng.randrange(2, p)))
        ha = tuple(HOWS[(i >> s) % 3] for s in (0, 1, 2, 3)) if i % 2 == 0 else tuple(rng.choice(HOWS) for _ in range(4))
        hb = tuple(HOWS[(i + 1 + (i >> s)) % 3] for s in (0, 1, 2, 3))
        if mu == 1:
            hb = hb[:2] + (0, 0)            # zz = zzz = 1: the canonical representative only
        rows.append(X.stored(curve, P, lam, ha, rng) + X.stored(curve, Q, mu, hb, rng))
    return rows


def replicated(out):
    assert (out == out[:, :1, :]).all(), np.argwhere((out != out[:, :1, :]).any(axis=(1, 2)))[:8]
    return out[:, 0, :].tolist()


@pytest.mark.parametrize("name", list(R.CURVES))
def test_quad_ops_on_affine_points_against_big_integers(h2, name):
    lib, c = h2.load(), R.CURVES[name]
    Ps, Qs, _ = pairs(c)

    def aff(pts):
        return np.frombuffer(b"".join(c.affine_bytes(P) for P in pts), dtype=np.uint64).reshape(len(pts), 8).copy()

    p, q = aff(Ps), aff(Qs)
    out = np.zeros_like(p)
    dbl = [c.add(a, a) for a in Ps]
    for op, want in ((0, [c.add(a, b) for a, b in zip(Ps, Qs)]), (1, dbl), (4, [c.add(d, b) for d, b in zip(dbl, Qs)])):
        assert lib.h2_selftest_curve_op_device(c.cid, op, p.ctypes.data, q.ctypes.data, out.ctypes.data, N) == 0
        assert np.array_equal(out, aff(want)), (name, op, np.argwhere((out != aff(want)).any(axis=1))[:8])


@pytest.mark.parametrize("name", list(R.CURVES))
def test_quad_ops_on_stored_points_replicated_in_range_and_the_models_limbs(h2, name):
    lib, c = h2.load(), R.CURVES[name]
    Ps, Qs, rng = pairs(c)
    rows = stored_rows(c, Ps, Qs, rng)
    chk = R.Fe29Check(c.base.p)

    def run(op, rows, want):
        got = replicated(X.device_rows(lib, c.cid, op, rows))
        for i in range(len(rows)):
            assert got[i] == X.model_row(name, op, rows[i], chk), (name, op, i)
            err = X.check_result(c, got[i], want[i])
            assert err is None, (name, op, i, err)
        return got

    added = run(X.ADD_QUAD, rows, [c.add(a, b) for a, b in zip(Ps, Qs)])
    dbl = [c.add(a, a) for a in Ps]
    doubled = run(X.DOUBLE_QUAD, rows, dbl)
    # the addition behind a doubling: operand A is the device's own 2 P
    run(X.ADD_QUAD, [d + r[36:] for d, r in zip(doubled, rows)], [c.add(d, b) for d, b in zip(dbl, Qs)])
    # the identity that P - P returned, as the device wrote it, on either side of the next addition
    for i in range(8, 16):
        assert not any(added[i][18:27]), i
    fresh = [X.stored(c, Qs[i + 24], rng.randrange(2, c.base.p), ("rand",) * 4, rng) for i in range(8, 16)]
    run(X.ADD_QUAD, [added[i] + f for i, f in zip(range(8, 16), fresh)], [Qs[i + 24] for i in range(8, 16)])
    run(X.ADD_QUAD, [f + added[i] for i, f in zip(range(8, 16), fresh)], [Qs[i + 24] for i in range(8, 16)])
    assert chk.max_product <= 64 and chk.max_zero_test < 16
