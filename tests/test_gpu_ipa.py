"""GPU: h2_ipa_* -- the rounds of the inner product argument on the registered table, held against upstream's LITERAL
algorithm round by round.

The reference below is the collapsing form of halo2_proofs' poly/ipa/commitment/prover.rs, not the expanded one the
library runs: a, b and f are Python integers, the generators G' are really folded every round (G'[i] += [u_j] G'[i + half]
with the C oracle's scale_points / jac_add / to_affine), and L_j, R_j are the C oracle's best_multiexp over the folded
generators, U and W.  Affine coordinates are canonical, so L_j || R_j is compared byte for byte in every round, and so are
c, b[0] and the finished table s."""
import ctypes
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CID = {"bn254": 0, "pallas": 1, "vesta": 2}
CURVES = ["bn254", "pallas", "vesta"]
H2_OK, H2_EINVAL = 0, -1


def L():
    from halo2_prover_amd import lib
    return lib.load()


def primes(curve):
    from halo2_prover_amd.transcript import FIELDS
    return FIELDS[CID[curve]][:2]


def limbs(values):
    buf = b"".join(int(v).to_bytes(32, "little") for v in values)
    return np.frombuffer(buf, dtype=np.uint64).reshape(-1, 4).copy()


def mont(p, values):
    R = (1 << 256) % p
    return limbs([v % p * R % p for v in values])


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64).copy()).cuda()


def from_dev(t):
    return t.cpu().numpy().view(np.uint64)


_SETUPS = {}


def setup(curve, k):
    """bases of one (curve, k): G (n points), U, W from the oracle's generator, registered once as G || U || W"""
    key = (curve, k)
    if key not in _SETUPS:
        import halo2_prover_amd as h2
        import oracle_lib as O
        h2.init(0)
        n = 1 << k
        pts = O.synth_bases(CID[curve], 0x49504100 + 16 * k + CID[curve], n + 2).reshape(n + 2, 8)
        _SETUPS[key] = {"g": pts[:n].copy(), "u": pts[n].copy(), "w": pts[n + 1].copy(), "bases": h2.Bases(curve, pts),
                        "short": None}
    return _SETUPS[key]


def jac_of(curve, aff):
    """affine (identity = zeros) -> Jacobian with Z = 1"""
    _, q = primes(curve)
    aff = np.asarray(aff, dtype=np.uint64).reshape(-1, 8)
    one = limbs([(1 << 256) % q])[0]
    out = np.zeros((aff.shape[0], 12), dtype=np.uint64)
    for i, pt in enumerate(aff):
        if pt.any():
            out[i, :8] = pt
            out[i, 8:] = one
    return out


def reference(curve, k, a, x3, z, us, blinds):
    """upstream's rounds, literally -> ([L_j || R_j affine limbs], c, b0, s)"""
    import oracle_lib as O
    from halo2_prover_amd.ipa import compute_s
    cid = CID[curve]
    p, _ = primes(curve)
    S = setup(curve, k)
    a = [v % p for v in a]
    b = [pow(x3, i, p) for i in range(1 << k)]
    G = S["g"].copy()
    out = []
    for j in range(k):
        half = 1 << (k - j - 1)
        l_j, r_j = blinds[j]
        ipl = sum(x * y for x, y in zip(a[half:], b[:half])) % p
        ipr = sum(x * y for x, y in zip(a[:half], b[half:])) % p
        lr = []
        for sc, gs, ip, bl in ((a[half:], G[:half], ipl, l_j), (a[:half], G[half:], ipr, r_j)):
            scalars = mont(p, list(sc) + [z * ip % p, bl])
            bases = np.concatenate([gs, S["u"].reshape(1, 8), S["w"].reshape(1, 8)])
            lr.append(O.to_affine(cid, O.best_multiexp(cid, scalars, bases)))
        out.append(np.concatenate(lr))
        u = us[j]
        ui = pow(u, -1, p)
        a = [(a[i] + a[i + half] * ui) % p for i in range(half)]
        b = [(b[i] + b[i + half] * u) % p for i in range(half)]
        hi = O.scale_points(cid, mont(p, [u])[0], jac_of(curve, G[half:])).reshape(half, 12)
        lo = jac_of(curve, G[:half])
        G = O.to_affine(cid, np.concatenate([O.jac_add(cid, lo[i], hi[i]) for i in range(half)])).reshape(half, 8)
    return out, a[0], b[0], compute_s(us, 1, p)


class Opening:
    """one caller-owned state buffer, reused by every run on it without being cleared"""

    def __init__(self, curve, k):
        import torch
        self.curve, self.k = curve, k
        need = ctypes.c_size_t(0)
        assert L().h2_ipa_state_bytes(k, ctypes.byref(need)) == H2_OK
        self.state = torch.full((need.value // 8,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
        self.out = torch.zeros(16, dtype=torch.int64, device="cuda")
        self.s_out = torch.zeros((1 << k, 4), dtype=torch.int64, device="cuda")

    def round(self, j, z, us, blinds, handle=None, state_ptr=None, drop_u=False):
        p, _ = primes(self.curve)
        S = setup(self.curve, self.k)
        um = mont(p, [us[j - 1], pow(us[j - 1], -1, p)]) if j and not drop_u else None
        zm, bm = mont(p, [z]), mont(p, blinds[min(j, self.k - 1)])
        return L().h2_ipa_round_device(CID[self.curve], S["bases"].handle if handle is None else handle, self.k, j,
                                       ctypes.c_void_p(self.state.data_ptr() if state_ptr is None else state_ptr),
                                       um[0].ctypes.data if um is not None else None,
                                       um[1].ctypes.data if um is not None else None, zm.ctypes.data, bm[0].ctypes.data,
                                       bm[1].ctypes.data, ctypes.c_void_p(self.out.data_ptr()), None)

    def run(self, a, x3, z, us, blinds):
        p, _ = primes(self.curve)
        cid, k = CID[self.curve], self.k
        d_p = to_dev(mont(p, a))
        before = from_dev(d_p).copy()
        assert L().h2_ipa_begin_device(cid, k, ctypes.c_void_p(d_p.data_ptr()), mont(p, [x3]).ctypes.data,
                                       ctypes.c_void_p(self.state.data_ptr()), None) == H2_OK
        got = []
        for j in range(k):
            assert self.round(j, z, us, blinds) == H2_OK
            got.append(from_dev(self.out).copy())
        um = mont(p, [us[-1], pow(us[-1], -1, p)])
        assert L().h2_ipa_final_device(cid, k, ctypes.c_void_p(self.state.data_ptr()), um[0].ctypes.data, um[1].ctypes.data,
                                       ctypes.c_void_p(self.out.data_ptr()), ctypes.c_void_p(self.s_out.data_ptr()),
                                       None) == H2_OK
        cb = from_dev(self.out)[:8].copy()
        assert np.array_equal(from_dev(d_p), before), "d_p is only read"
        return got, cb, from_dev(self.s_out).copy()


def check(op, a, x3, z, us, blinds):
    p, _ = primes(op.curve)
    want_lr, c, b0, s = reference(op.curve, op.k, a, x3, z, us, blinds)
    got_lr, cb, s_got = op.run(a, x3, z, us, blinds)
    for j, (g, w) in enumerate(zip(got_lr, want_lr)):
        assert np.array_equal(g[:8], w[:8]), "L_%d differs" % j
        assert np.array_equal(g[8:], w[8:]), "R_%d differs" % j
    assert np.array_equal(cb.reshape(2, 4), mont(p, [c, b0])), "c or b[0] differs"
    assert np.array_equal(s_got, mont(p, s)), "the finished s differs"
    return got_lr


def inputs(curve, k, seed):
    p, _ = primes(curve)
    rnd = random.Random(seed)
    n = 1 << k
    return {"a": [rnd.randrange(p) for _ in range(n)], "x3": rnd.randrange(1, p), "z": rnd.randrange(1, p),
            "us": [rnd.randrange(1, p) for _ in range(k)],
            "blinds": [(rnd.randrange(p), rnd.randrange(p)) for _ in range(k)]}


@pytest.mark.parametrize("k", [1, 2, 3, 6])
@pytest.mark.parametrize("curve", CURVES)
def test_rounds_match_the_collapsing_algorithm(curve, k):
    check(Opening(curve, k), **inputs(curve, k, 0x1A0 + k))


def test_more_than_one_workgroup_on_pallas():
    check(Opening("pallas", 10), **inputs("pallas", 10, 0x10A))


@pytest.mark.parametrize("k", [3, 6])
@pytest.mark.parametrize("case", ["zero_a_blinds", "zero_a_zero_blinds", "u_one", "u_minus_one", "upper_half_zero",
                                  "lower_half_zero", "z_zero"])
def test_edge_inputs(case, k):
    import oracle_lib as O
    curve = "pallas"
    p, _ = primes(curve)
    n = 1 << k
    I = inputs(curve, k, 0xED6E + k)
    if case.startswith("zero_a"):
        I["a"] = [0] * n
    if case == "zero_a_zero_blinds":
        I["blinds"] = [(0, 0)] * k
    if case == "u_one":
        I["us"] = [1] * k
    if case == "u_minus_one":
        I["us"] = [p - 1] * k
    if case == "upper_half_zero":
        I["a"][n // 2:] = [0] * (n // 2)
    if case == "lower_half_zero":
        I["a"][:n // 2] = [0] * (n // 2)
    if case == "z_zero":
        I["z"] = 0
    got = check(Opening(curve, k), **I)
    if case == "zero_a_blinds":                       # L_j = [l_j] W
        S = setup(curve, k)
        for j in range(k):
            want = O.to_affine(1, O.scalar_mul(1, mont(p, [I["blinds"][j][0]])[0], S["w"]))
            assert np.array_equal(got[j][:8], want)
    if case == "zero_a_zero_blinds":                  # the identity comes out as (0, 0)
        assert all(not g.any() for g in got)


@pytest.mark.parametrize("k", [3, 6])
def test_a_second_opening_on_the_same_state_sees_nothing_stale(k):
    op = Opening("vesta", k)
    check(op, **inputs("vesta", k, 0x57A1E))
    check(op, **inputs("vesta", k, 0x57A1F))          # a different polynomial, the state not cleared in between


@pytest.mark.parametrize("curve,k", [("bn254", 1), ("pallas", 3), ("vesta", 6), ("pallas", 10)])
def test_challenge_products_against_compute_s(curve, k):
    import torch
    from halo2_prover_amd.ipa import compute_s
    p, _ = primes(curve)
    rnd = random.Random(0xC5 + k)
    us = [rnd.randrange(1, p) for _ in range(k)]
    init = rnd.randrange(2, p)
    setup(curve, k)
    n = 1 << k
    buf = torch.full((n + 2, 4), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    um = mont(p, us)
    assert L().h2_ipa_challenge_products_device(CID[curve], um.ctypes.data, k, mont(p, [init]).ctypes.data,
                                                ctypes.c_void_p(buf.data_ptr()), None) == H2_OK
    got = from_dev(buf)
    assert np.array_equal(got[:n], mont(p, compute_s(us, init, p)))
    assert (got[n:] == 0x5A5A5A5A5A5A5A5A).all(), "written past the 2^k products"


def test_argument_errors_then_a_valid_call():
    import halo2_prover_amd as h2
    curve, k = "pallas", 3
    p, _ = primes(curve)
    S = setup(curve, k)
    I = inputs(curve, k, 0xE44)
    op = Opening(curve, k)
    check(op, **I)
    short = h2.Bases(curve, np.concatenate([S["g"]]))                    # 2^k bases instead of 2^k + 2
    other = setup("vesta", k)["bases"]                                   # the right size, another curve
    z, us, bl = I["z"], I["us"], I["blinds"]
    assert op.round(0, z, us, bl, handle=short.handle) == H2_EINVAL
    assert op.round(0, z, us, bl, handle=other.handle) == H2_EINVAL
    assert op.round(k, z, us, bl) == H2_EINVAL                           # j = k
    assert op.round(1, z, us, bl, drop_u=True) == H2_EINVAL              # u_prev missing at j = 1
    assert op.round(0, z, us, bl, state_ptr=op.state.data_ptr() + 8) == H2_EINVAL    # misaligned
    um = mont(p, [us[0], pow(us[0], -1, p)])
    zm, bm = mont(p, [z]), mont(p, bl[0])
    assert L().h2_ipa_round_device(1, S["bases"].handle, k, 0, ctypes.c_void_p(op.state.data_ptr()), um[0].ctypes.data,
                                   um[1].ctypes.data, zm.ctypes.data, bm[0].ctypes.data, bm[1].ctypes.data,
                                   ctypes.c_void_p(op.out.data_ptr()), None) == H2_EINVAL     # superfluous u_prev at j = 0
    assert L().h2_ipa_begin_device(7, k, ctypes.c_void_p(op.state.data_ptr()), zm.ctypes.data,
                                   ctypes.c_void_p(op.state.data_ptr()), None) == H2_EINVAL   # unknown curve
    short.release()
    check(op, **I)                                                       # the next valid opening still gives the right bytes
