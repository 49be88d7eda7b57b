"""ipa.verify_proofs and h2_ipa_challenge_products_sum_device on the GPU: the sum kernel against compute_s, and the batch
verifier against ipa.verify_proof item by item -- good batches, every kind of bad item, the bisection's check count, the
weights, and where the transcripts are left."""
import math
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

    def __init__(self, seed, prefix=b""):
        self.r, self.prefix, self.draws = random.Random(seed), prefix, 0

    def __call__(self, n):
        self.draws += 1
        if self.prefix:
            out, self.prefix = self.prefix[:n], self.prefix[n:]
            return out
        return bytes(self.r.getrandbits(8) for _ in range(n))


_BATCH = {}


def batch(curve, k, count):
    """params and `count` proofs under them, each of its own polynomial, blind and point: shared by the tests, never changed"""
    key = (curve, k)
    if key not in _BATCH:
        import halo2_prover_amd as h2
        import oracle_lib as O
        from halo2_prover_amd import ipa
        h2.init(0)
        cid, n = CID[curve], 1 << k
        pts = O.synth_bases(cid, 0x49564200 + 16 * k + cid, n + 2).reshape(n + 2, 8)
        _BATCH[key] = dict(curve=curve, k=k, params=ipa.ParamsIPA(curve, k, pts[:n], pts[n + 1], pts[n]), proofs=[])
    B = _BATCH[key]
    import halo2_prover_amd as h2
    from halo2_prover_amd import ipa
    params = B["params"]
    p, n = params.p, 1 << k
    R = (1 << 256) % p
    while len(B["proofs"]) < count:
        i = len(B["proofs"])
        rnd = random.Random(0xBA7C4 + 64 * k + i)
        poly = [rnd.randrange(p) for _ in range(n)]
        blind, x3 = rnd.randrange(p), rnd.randrange(1, p)
        poly_m = limbs([c * R % p for c in poly])
        v = sum(c * pow(x3, j, p) for j, c in enumerate(poly)) % p
        proof = ipa.create_proof(params, h2.Blake2bTranscript(curve), poly_m, blind, x3, Rng(100 + i))
        B["proofs"].append(dict(P=params.commit(poly_m, blind), x3=x3, v=v, proof=proof))
    return B


def run(B, entries, rng=None, prefix=b"junk"):
    """verify_proofs and, item by item, verify_proof on fresh transcripts that start behind `prefix` -> (batch verdicts, single
    verdicts, stats, the batch's transcripts, the single calls' transcripts)"""
    import halo2_prover_amd as h2
    from halo2_prover_amd import ipa

    def transcripts():
        out = []
        for e in entries:
            tr = h2.Blake2bTranscript(B["curve"], prefix + e["proof"])
            tr.pos = len(prefix)
            out.append(tr)
        return out
    stats = {}
    tb, ts = transcripts(), transcripts()
    got = ipa.verify_proofs(B["params"], [(t, e["P"], e["x3"], e["v"]) for t, e in zip(tb, entries)], rng=rng or Rng(5), stats=stats)
    single = [ipa.verify_proof(B["params"], t, e["P"], e["x3"], e["v"]) for t, e in zip(ts, entries)]
    for a, b in zip(tb, ts):                                   # left where verify_proof leaves them, the hash state included
        assert a.pos == b.pos and a.state.digest() == b.state.digest()
    return got, single, stats, tb, ts


def flip(proof, byte, bit=0):
    out = bytearray(proof)
    out[byte] ^= 1 << bit
    return bytes(out)


# ------------------------------------------------------------------------------------------------ the sum kernel ----
@pytest.mark.parametrize("k", [1, 3, 5, 9, 13])
def test_sum_kernel_matches_compute_s(h2, k):
    import torch
    from halo2_prover_amd import ipa
    from halo2_prover_amd.transcript import FIELDS
    p, n = FIELDS[1][0], 1 << k
    R_inv = pow(1 << 256, -1, p)
    rnd = random.Random(0x53554D + k)
    u = [[rnd.randrange(p) for _ in range(k)] for _ in range(33)]
    init = [rnd.randrange(p) for _ in range(33)]
    vectors = [ipa.compute_s(u[i], init[i], p) for i in range(33)]
    for count in (1, 2, 5, 33):
        out = torch.full((n + 1, 4), -1, dtype=torch.int64, device="cuda")
        ipa.challenge_products_sum("pallas", k, u[:count], init[:count], out=out)
        raw = out.cpu().numpy().view(np.uint64)
        assert (raw[n] == np.uint64(0xFFFFFFFFFFFFFFFF)).all()                      # nothing written behind 2^k elements
        got = [int.from_bytes(raw[i].tobytes(), "little") for i in range(n)]
        assert all(g < p for g in got)                                               # canonical, so bit for bit
        want = [sum(vec[i] for vec in vectors[:count]) % p for i in range(n)]
        assert [g * R_inv % p for g in got] == want, (k, count)
    out = torch.full((n, 4), -1, dtype=torch.int64, device="cuda")
    ipa.challenge_products_sum("pallas", k, [], [], out=out)
    assert not out.cpu().numpy().any()                                               # count = 0 writes zeros


def test_sum_kernel_runs_group_after_group(h2):
    """more proofs than one launch takes (65535): the later group adds into what the first one stored"""
    from halo2_prover_amd import ipa
    from halo2_prover_amd.transcript import FIELDS
    p, k, count = FIELDS[1][0], 1, 65535 + 3
    R_inv = pow(1 << 256, -1, p)
    rnd = random.Random(0x47525550)
    u = [[rnd.randrange(p)] for _ in range(count)]
    init = [rnd.randrange(p) for _ in range(count)]
    raw = ipa.challenge_products_sum("pallas", k, u, init).cpu().numpy().view(np.uint64)
    got = [int.from_bytes(raw[i].tobytes(), "little") for i in range(2)]
    assert all(g < p for g in got)
    assert [g * R_inv % p for g in got] == [sum(init) % p, sum(a * b[0] for a, b in zip(init, u)) % p]


def test_sum_kernel_argument_checks(h2):
    import torch
    L = h2.load()
    buf = torch.zeros(1024, dtype=torch.int64, device="cuda")
    u = limbs([1, 2, 3, 4])
    fn = L.h2_ipa_challenge_products_sum_device
    assert fn(1, u.ctypes.data, u.ctypes.data, 0, 1, buf.data_ptr(), None) == -1     # k = 0
    assert fn(1, u.ctypes.data, u.ctypes.data, 21, 1, buf.data_ptr(), None) == -1    # k > H2_IPA_MAX_K
    assert fn(3, u.ctypes.data, u.ctypes.data, 4, 1, buf.data_ptr(), None) == -1     # unknown curve
    assert fn(1, None, u.ctypes.data, 4, 1, buf.data_ptr(), None) == -1              # null u / init with count > 0
    assert fn(1, u.ctypes.data, None, 4, 1, buf.data_ptr(), None) == -1
    assert fn(1, u.ctypes.data, u.ctypes.data, 4, 1, None, None) == -1
    assert fn(1, u.ctypes.data, u.ctypes.data, 4, 1, buf.data_ptr() + 8, None) == -1  # not 16-byte aligned
    assert fn(1, None, None, 4, 0, buf.data_ptr(), None) == 0
    torch.cuda.synchronize()


# --------------------------------------------------------------------------------------------------- verify_proofs ----
@pytest.mark.parametrize("curve,k,N", [("pallas", 4, 5), ("vesta", 4, 5), ("pallas", 8, 3), ("vesta", 8, 3)])
def test_good_batch(h2, curve, k, N):
    B = batch(curve, k, N)
    got, single, stats, tb, _ = run(B, B["proofs"][:N])
    assert got == single == [True] * N
    assert stats == {"checks": 1, "points": N * (2 * k + 1), "rejected_early": 0}
    assert all(t.pos == 4 + 32 * (2 * k + 3) for t in tb)


def off_curve_x(params, start):
    """bytes of an x in range with no point on the curve"""
    from halo2_prover_amd.transcript import sqrt_mod
    x = start
    while sqrt_mod(x * x * x + 5, params.q) is not None:
        x += 1
    return x.to_bytes(32, "little")


def on_curve_bit_flip(params, proof, at):
    """the proof with one low bit of the x at byte offset `at` flipped so that the new x is still on the curve"""
    from halo2_prover_amd.transcript import TranscriptError, decompress
    for bit in range(64):
        cand = flip(proof, at + bit // 8, bit % 8)
        try:
            if decompress(params.curve, cand[at:at + 32]) is not None:
                return cand
        except TranscriptError:
            pass
    raise AssertionError("no bit keeps the point on the curve")


KINDS = ["bit of c", "bit of L_j on the curve", "L_j off the curve", "wrong v", "cut short", "S is 32 zero bytes"]


@pytest.mark.parametrize("kind", KINDS)
def test_one_bad_item_among_five(h2, kind):
    k = 4
    B = batch("pallas", k, 5)
    params = B["params"]
    entries = [dict(e) for e in B["proofs"][:5]]
    bad = entries[2]
    proof = bad["proof"]
    lj = 32 * (1 + 2 * 1)                                        # L_1
    if kind == "bit of c":
        bad["proof"] = flip(proof, 32 * (2 * k + 1) + 3, 2)
    elif kind == "bit of L_j on the curve":
        bad["proof"] = on_curve_bit_flip(params, proof, lj)
    elif kind == "L_j off the curve":
        bad["proof"] = proof[:lj] + off_curve_x(params, int.from_bytes(proof[lj:lj + 31], "little")) + proof[lj + 32:]
    elif kind == "wrong v":
        bad["v"] = (bad["v"] + 1) % params.p
    elif kind == "cut short":
        bad["proof"] = proof[:32 * (2 * k + 2) + 7]
    else:
        bad["proof"] = bytes(32) + proof[32:]
    got, single, stats, _, _ = run(B, entries)
    assert got == single == [True, True, False, True, True], kind
    assert stats["rejected_early"] == (1 if kind in ("L_j off the curve", "cut short") else 0)


def test_bisection(h2):
    k = 4
    B = batch("pallas", k, 8)
    good = B["proofs"][:8]

    def spoiled(which):
        return [dict(e, v=(e["v"] + 1) % B["params"].p) if i in which else e for i, e in enumerate(good)]
    got, single, stats, _, _ = run(B, spoiled({1, 6}))
    assert got == single == [i not in (1, 6) for i in range(8)]
    assert stats["checks"] <= 1 + 2 * 2 * math.ceil(math.log2(8))        # the halving bound: two checks per level and culprit
    got, single, stats, _, _ = run(B, spoiled(set(range(8))))
    assert got == single == [False] * 8
    for entries, want in ((good[:1], [True]), (spoiled({0})[:1], [False])):
        got, single, stats, _, _ = run(B, entries)
        assert got == single == want and stats["checks"] == 1
    stats = {}
    from halo2_prover_amd import ipa
    assert ipa.verify_proofs(B["params"], [], stats=stats) == [] and stats == {"checks": 0, "points": 0, "rejected_early": 0}


def test_weights(h2):
    B = batch("pallas", 4, 5)
    entries = [dict(e) for e in B["proofs"][:5]]
    entries[3]["v"] = (entries[3]["v"] + 1) % B["params"].p
    first = run(B, entries, rng=Rng(11))[0]
    assert first == run(B, entries, rng=Rng(11))[0] == [True, True, True, False, True]
    # a zero weight would make the bad item invisible to the first check: it is redrawn, not used
    rng = Rng(12, prefix=bytes(16))
    got, single, stats, _, _ = run(B, entries[3:4], rng=rng)
    assert got == single == [False] and rng.draws == 2 and stats["checks"] == 1


def test_bn254_params_are_refused(h2):
    import oracle_lib as O
    from halo2_prover_amd import ipa
    pts = O.synth_bases(0, 0x49564201, 6).reshape(6, 8)
    params = ipa.ParamsIPA("bn254", 2, pts[:4], pts[5], pts[4])
    with pytest.raises(ValueError):
        ipa.verify_proofs(params, [])
