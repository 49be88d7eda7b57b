"""GPU: the inner product argument end to end -- ipa.create_proof's bytes are accepted by a verifier written here that
makes no GPU call (the transcript replayed in Python, the final equation on Python integers and the C oracle's
best_multiexp), the same verifier rejects tampered proofs and a wrong value, and ipa.verify_proof agrees with it.

There are no recorded upstream bytes for this argument: the reference proves with KZG only.  The pins are the parity with
the literal algorithm (test_gpu_ipa.py) and the verification equation
    sum [u_j^-1] L_j + P - [v] G[0] + [xi] S + sum [u_j] R_j == [c] <s, G> + [c b_0 z] U + [f] W."""
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CID = {"pallas": 1, "vesta": 2}


def limbs(values):
    buf = b"".join(int(v).to_bytes(32, "little") for v in values)
    return np.frombuffer(buf, dtype=np.uint64).reshape(-1, 4).copy()


class Rng:
    """a deterministic callable n -> n bytes"""

    def __init__(self, seed):
        self.r = random.Random(seed)

    def __call__(self, n):
        return bytes(self.r.getrandbits(8) for _ in range(n))


_CASES = {}


def case(curve, k):
    """params, a polynomial, its blind, commitment, point and value, and ONE proof: shared by the tests, never changed"""
    key = (curve, k)
    if key not in _CASES:
        import halo2_prover_amd as h2
        import oracle_lib as O
        from halo2_prover_amd import ipa
        h2.init(0)
        cid, n = CID[curve], 1 << k
        pts = O.synth_bases(cid, 0x49504200 + 16 * k + cid, n + 2).reshape(n + 2, 8)
        params = ipa.ParamsIPA(curve, k, pts[:n], pts[n + 1], pts[n])
        p = params.p
        rnd = random.Random(0xA11CE + k + cid)
        poly = [rnd.randrange(p) for _ in range(n)]
        blind, x3 = rnd.randrange(p), rnd.randrange(1, p)
        s_poly = [rnd.randrange(p) for _ in range(n)]
        R = (1 << 256) % p
        poly_m, s_m = limbs([c * R % p for c in poly]), limbs([c * R % p for c in s_poly])
        v = sum(c * pow(x3, i, p) for i, c in enumerate(poly)) % p
        commitment = params.commit(poly_m, blind)
        proof = ipa.create_proof(params, h2.Blake2bTranscript(curve), poly_m, blind, x3, Rng(7), s_poly=s_m)
        _CASES[key] = dict(curve=curve, k=k, params=params, pts=pts, poly=poly, poly_m=poly_m, s_m=s_m, blind=blind, x3=x3, v=v,
                           P=commitment, proof=proof)
    return _CASES[key]


def host_verify(C, proof, v):
    """no GPU call: Python transcript, Python integers, the C oracle's best_multiexp"""
    import oracle_lib as O
    from halo2_prover_amd.ipa import compute_b, compute_s
    from halo2_prover_amd.transcript import Blake2bTranscript, TranscriptError
    params, k, cid = C["params"], C["k"], CID[C["curve"]]
    p, q = params.p, params.q
    n = 1 << k
    tr = Blake2bTranscript(C["curve"], proof)
    try:
        S = tr.read_point()
        xi, z = tr.squeeze_challenge(), tr.squeeze_challenge()
        rounds = []
        for _ in range(k):
            lp, rp = tr.read_point(), tr.read_point()
            rounds.append((lp, rp, tr.squeeze_challenge()))
        c, f = tr.read_scalar(), tr.read_scalar()
    except TranscriptError:
        return False
    if tr.pos != len(proof):
        return False
    u = [r[2] for r in rounds]
    s = compute_s(u, 1, p)
    b0 = compute_b(C["x3"], u, p)
    R, Rq = (1 << 256) % p, (1 << 256) % q

    def aff(pt):
        x, y = pt if pt is not None else (0, 0)
        return limbs([x * Rq % q, y * Rq % q]).reshape(8)

    # left - right == identity
    scalars = [(-c * si) % p for si in s] + [(-c * b0 * z) % p, (-f) % p]
    scalars[0] = (scalars[0] - v) % p
    bases = [C["pts"][i] for i in range(n + 2)]
    extra = [(1, C["P"]), (xi, S)]
    for lp, rp, uj in rounds:
        extra += [(pow(uj, -1, p), lp), (uj, rp)]
    for sc, pt in extra:
        if pt is not None:
            scalars.append(sc % p)
            bases.append(aff(pt))
    total = O.to_affine(cid, O.best_multiexp(cid, limbs([x * R % p for x in scalars]), np.stack(bases)))
    return not total.any()


def flip(proof, byte, bit=0):
    out = bytearray(proof)
    out[byte] ^= 1 << bit
    return bytes(out)


def both(C, proof, v):
    import halo2_prover_amd as h2
    from halo2_prover_amd import ipa
    mine = host_verify(C, proof, v)
    theirs = ipa.verify_proof(C["params"], h2.Blake2bTranscript(C["curve"], proof), C["P"], C["x3"], v)
    assert mine == theirs, "ipa.verify_proof disagrees with the host verifier"
    return mine


@pytest.mark.parametrize("k", [4, 8])
@pytest.mark.parametrize("curve", ["pallas", "vesta"])
def test_the_proof_verifies(curve, k):
    C = case(curve, k)
    assert len(C["proof"]) == 32 * (1 + 2 * k + 2)
    assert both(C, C["proof"], C["v"])


@pytest.mark.parametrize("k", [4, 8])
@pytest.mark.parametrize("curve", ["pallas", "vesta"])
def test_tampered_proofs_and_a_wrong_value_are_rejected(curve, k):
    C = case(curve, k)
    proof = C["proof"]
    assert not both(C, flip(proof, 32 * (1 + 2 * k)), C["v"])               # one bit of c
    assert not both(C, flip(proof, 32 * (1 + 2 * (k // 2)) + 3, 2), C["v"])   # one bit of an L_j
    assert not both(C, proof, (C["v"] + 1) % C["params"].p)                 # a wrong v


@pytest.mark.parametrize("curve,k", [("pallas", 4), ("vesta", 8)])
def test_explicit_s_poly_and_a_deterministic_rng_give_identical_bytes(curve, k):
    import halo2_prover_amd as h2
    from halo2_prover_amd import ipa
    C = case(curve, k)
    again = ipa.create_proof(C["params"], h2.Blake2bTranscript(curve), C["poly_m"], C["blind"], C["x3"], Rng(7), s_poly=C["s_m"])
    assert again == C["proof"]


def test_s_poly_drawn_on_the_device_verifies_too():
    import halo2_prover_amd as h2
    from halo2_prover_amd import ipa
    C = case("pallas", 4)
    proof = ipa.create_proof(C["params"], h2.Blake2bTranscript("pallas"), C["poly_m"], C["blind"], C["x3"], Rng(11))
    assert proof != C["proof"] and both(C, proof, C["v"])


@pytest.mark.parametrize("curve,k", [("pallas", 4), ("vesta", 8)])
def test_commit_is_the_oracles_msm_plus_the_blinded_w(curve, k):
    import oracle_lib as O
    C = case(curve, k)
    cid, params = CID[curve], C["params"]
    p = params.p
    R = (1 << 256) % p
    n = 1 << k
    msm = O.best_multiexp(cid, C["poly_m"], C["pts"][:n])
    rw = O.scalar_mul(cid, limbs([C["blind"] * R % p])[0], C["pts"][n + 1])
    want = O.to_affine(cid, O.jac_add(cid, msm, rw))
    assert np.array_equal(params.affine_limbs(C["P"]), want)
