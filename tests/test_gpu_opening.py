"""GPU: the multiopen argument's columns through h2_poly_lincomb_device (halo2_prover_amd/opening.py), BN254.

gwc_open, shplonk_open_h and shplonk_open_final against the schemes recomputed in Python integers: SHPLONK by
oracle/halo2_ref.py's shplonk_open itself (its transcript and commitments replaced by recorders), GWC by its definition
on the oracle's polynomial helpers.  Field results are canonical, so the device columns must agree exactly.  Each of the
three is ONE h2_poly_lincomb_device call (counted by wrapping the loaded symbol), and halo2_prover_amd.prover reaches the
recorded proof bytes through them without a single scale of its own during the multiopen."""
import os
import random

import numpy as np
import pytest

import halo2_ref as H
import pyref as R

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
P = H.P
K, N = 6, 64


class SurveyRng:
    """the deterministic stream of SURVEY.md App. B.2"""

    def __init__(self, start=0):
        self.s = R.SurveyStream(start=start)

    def fill(self, n):
        return self.s.fill(n)

    def fr_random(self, _field=None):
        return self.s.fr_random(R.BN_FR)


@pytest.fixture()
def calls(h2, monkeypatch):
    """every h2_poly_lincomb_device call and every _Dev.scale of the prover, in order"""
    from halo2_prover_amd import prover
    lib = h2.load()
    real = lib.h2_poly_lincomb_device
    events = []

    def counted(*args):
        events.append("lincomb")
        return real(*args)
    monkeypatch.setattr(lib, "h2_poly_lincomb_device", counted)
    real_scale = prover._Dev.scale

    def scale(self, a, c):
        events.append("scale")
        return real_scale(self, a, c)
    monkeypatch.setattr(prover._Dev, "scale", scale)
    return events


@pytest.fixture(scope="module")
def case(h2):
    """eight random polynomials of 64 coefficients and queries at x, w x and w^-1 x that form rotation sets of one, two and
    three points; polynomial 0 is queried twice at the same point.  Computed once, never changed."""
    from halo2_prover_amd.domain import EvaluationDomain
    dom = EvaluationDomain(3, K, "bn254")
    rng = random.Random(0x4F50454E)
    polys = [[rng.randrange(P) for _ in range(N)] for _ in range(8)]
    x = rng.randrange(P)
    xn, xp = x * dom.omega % P, x * dom.omega_inv % P
    where = [(0, x), (3, x), (5, xn), (1, x), (5, x), (3, xn), (0, x), (4, xn), (6, xp), (4, x), (2, x), (5, xp), (6, x),
             (6, xn), (7, x)]
    Rm = (1 << 256) % P
    cols = [dom.to_device(np.frombuffer(b"".join((c * Rm % P).to_bytes(32, "little") for c in f), dtype=np.uint64).reshape(N, 4).copy())
            for f in polys]
    y, v, u = (rng.randrange(P) for _ in range(3))
    return {"dom": dom, "polys": polys, "cols": cols, "where": where, "y": y, "v": v, "u": u}


def ints_of(col):
    rinv = pow((1 << 256) % P, -1, P)
    raw = col.cpu().numpy().tobytes()
    return [int.from_bytes(raw[i:i + 32], "little") * rinv % P for i in range(0, len(raw), 32)]


def padded(f):
    return list(f) + [0] * (N - len(f))


class Recorder:
    """stands in for the oracle's transcript and its commitments: hands out the challenges, keeps what is committed"""

    def __init__(self, challenges):
        self.challenges, self.committed = list(challenges), []

    def squeeze(self):
        return self.challenges.pop(0)

    def write_point(self, pt):
        pass

    def commit(self, coeffs):
        self.committed.append(list(coeffs))


def test_rotation_sets_of_one_two_and_three(case):
    from halo2_prover_amd.opening import rotation_sets
    sets = rotation_sets([(pt, case["cols"][i], i) for i, pt in case["where"]])
    assert sorted(len(s) for s, _ in sets) == [1, 2, 3]
    assert sorted(len(m) for _, m in sets) == [2, 2, 4]


def test_gwc_open_is_the_definition(case, calls):
    from halo2_prover_amd import gwc_open
    v = case["v"]
    got = gwc_open(case["dom"], [(pt, case["cols"][i], i) for i, pt in case["where"]], v)
    assert calls == ["lincomb"]
    points = []
    for _, pt in case["where"]:
        if pt not in points:
            points.append(pt)
    assert got.shape == (3, N, 4)
    for j, pt in enumerate(points):
        acc, vp = [], 1
        for i, qpt in case["where"]:
            if qpt == pt:
                acc = H.padd(acc, H.pscale(case["polys"][i], vp))
                vp = vp * v % P
        assert ints_of(got[j]) == padded(H.pdiv_linear(acc, pt)), "witness %d" % j


def test_shplonk_open_is_the_oracles(case, calls):
    from halo2_prover_amd import shplonk_open_final, shplonk_open_h
    rec = Recorder([case["y"], case["v"], case["u"]])
    H.shplonk_open(rec, rec, [(pt, case["polys"][i]) for i, pt in case["where"]], {})
    want_h, want_w = rec.committed
    queries = [(pt, case["cols"][i], i) for i, pt in case["where"]]
    evals = {(i, pt): H.peval(case["polys"][i], pt) for i, pt in case["where"]}
    h, state = shplonk_open_h(case["dom"], queries, evals, case["y"], case["v"])
    assert calls == ["lincomb"]
    assert ints_of(h) == padded(want_h)
    w = shplonk_open_final(state, case["u"])
    assert calls == ["lincomb", "lincomb"]
    assert ints_of(w) == padded(want_w)


def no_scale_in_the_multiopen(events):
    """the prover's first lincomb call joins the quotient pieces, in front of the multiopen: no scale from there on"""
    assert "lincomb" in events
    assert "scale" not in events[events.index("lincomb"):]


def test_arithmetic_gwc_proof_through_the_call(h2, calls):
    from halo2_prover_amd import prover
    params = h2.ParamsKZG.read(open(os.path.join(GOLDEN, "params_k4.bin"), "rb").read())
    circuit = prover.ArithmeticCircuit.from_json('{"x":6,"y":9,"constant":7,"z":2923}')
    pk = prover.generate_keys(params, circuit)
    proof = prover.generate_proof_with_instance(params, pk, circuit, [7, 2923], SurveyRng(8))
    assert proof == open(os.path.join(GOLDEN, "proof_arithmetic_k4.bin"), "rb").read()
    assert calls.count("lincomb") == 2                       # h(X), the witnesses
    no_scale_in_the_multiopen(calls)


def test_collatz_shplonk_proof_through_the_call(h2, calls):
    from halo2_prover_amd import prover
    rng = SurveyRng(0)
    params = prover.generate_params(10, rng)
    seq = [9, 28, 14, 7, 22, 11, 34, 17, 52, 26, 13, 40, 20, 10, 5, 16, 8, 4, 2, 1]
    circuit = prover.CollatzCircuit(seq)
    pk = prover.generate_keys(params, circuit)
    proof = prover.generate_proof(params, pk, circuit, rng)
    assert proof == open(os.path.join(GOLDEN, "proof_collatz_k10.bin"), "rb").read()
    assert calls.count("lincomb") == 3                       # h(X) of the quotient, SHPLONK's h(X), its final quotient
    no_scale_in_the_multiopen(calls)
