"""GPU: EvaluationDomain pieces against the big-int restatement, bit for bit,
and through size-independent properties at k = 16.  The ZETA constant is recalled, not pinned by any reference
vector ("parity unpinned" for the coset choice; the polynomials it helps compute are unique)."""
import numpy as np
import pytest

import oracle_lib as O
import pyref as R

pytestmark = pytest.mark.gpu


def to_ints(f, t):
    a = t.cpu().numpy().view(np.uint64).reshape(-1, 4)
    return [f.from_mont(O.limbs_to_int(r)) for r in a]


def from_ints(f, dom, vals):
    return dom.to_device(np.array([f.limbs(v) for v in vals], dtype=np.uint64))


def horner(coeffs, x, p):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % p
    return acc


@pytest.mark.parametrize("curve,j,k", [("bn254", 3, 4), ("bn254", 4, 5), ("bn254", 6, 4), ("pallas", 6, 3), ("vesta", 4, 4)])
def test_domain_against_bigint(h2, curve, j, k):
    import torch
    from halo2_prover_amd.domain import EvaluationDomain
    f = R.CURVES[curve].scalar
    dom = EvaluationDomain(j, k, curve)
    p, n = f.p, 1 << k
    assert dom.omega == f.omega(k) and dom.extended_omega == f.omega(dom.extended_k)
    assert (1 << dom.extended_k) >= n * (j - 1) > (1 << (dom.extended_k - 1)) or dom.extended_k == k
    rng = R.SplitMix64(1000 * j + k)
    lagr = [R.synth_scalar(rng, p) for _ in range(n)]
    # lagrange_to_coeff == naive inverse DFT
    t = from_ints(f, dom, lagr)
    dom.lagrange_to_coeff(t)
    coeffs = to_ints(f, t)
    ninv = pow(n, -1, p)
    want = [x * ninv % p for x in R.dft_naive(lagr, pow(f.omega(k), -1, p), p)]
    assert coeffs == want
    assert [horner(coeffs, pow(f.omega(k), i, p), p) for i in range(n)] == lagr
    # coeff_to_extended: evaluations on the coset zeta * <extended_omega>
    ext = dom.coeff_to_extended(t)
    en = 1 << dom.extended_k
    got = to_ints(f, ext)
    assert got == [horner(coeffs, dom.g_coset * pow(dom.extended_omega, i, p) % p, p) for i in range(en)]
    # divide_by_vanishing_poly: multiply by 1 / (x^n - 1) on the coset
    ext2 = ext.clone()
    dom.divide_by_vanishing_poly(ext2)
    xs = [dom.g_coset * pow(dom.extended_omega, i, p) % p for i in range(en)]
    assert to_ints(f, ext2) == [g * pow((pow(x, n, p) - 1) % p, -1, p) % p for g, x in zip(got, xs)]
    # extended_to_coeff undoes coeff_to_extended (padded with zeros up to n*(j-1))
    back = to_ints(f, dom.extended_to_coeff(ext))
    assert back == (coeffs + [0] * (n * (j - 1)))[: n * (j - 1)]
    # pointwise ops and scaling
    a = from_ints(f, dom, lagr)
    b = from_ints(f, dom, coeffs)
    assert to_ints(f, dom.pointwise("mul", a.clone(), b)) == [x * y % p for x, y in zip(lagr, coeffs)]
    assert to_ints(f, dom.pointwise("add", a.clone(), b)) == [(x + y) % p for x, y in zip(lagr, coeffs)]
    assert to_ints(f, dom.pointwise("sub", a.clone(), b)) == [(x - y) % p for x, y in zip(lagr, coeffs)]
    assert to_ints(f, dom.scale(a.clone(), 12345)) == [x * 12345 % p for x in lagr]
    torch.cuda.synchronize()


def test_quotient_of_a_product_k16(h2):
    """size-independent property at the metric's size (k = 16, degree-3 domain): for random polynomials a, b of
    degree < n, h = (a*b - r) / (X^n - 1) computed with coset NTTs satisfies a*b = h*(X^n - 1) + r at a random
    point, where r = a*b mod (X^n - 1) is what the Lagrange-basis product gives."""
    import torch
    from halo2_prover_amd.domain import EvaluationDomain
    curve, j, k = "bn254", 3, 16
    f = R.CURVES[curve].scalar
    p, n = f.p, 1 << k
    dom = EvaluationDomain(j, k, curve)
    A = O.synth_scalars(1, 0x48324D5300000A01, n).reshape(n, 4)
    B = O.synth_scalars(1, 0x48324D5300000A02, n).reshape(n, 4)
    a_l, b_l = dom.to_device(A), dom.to_device(B)           # Lagrange values
    a_c, b_c = dom.lagrange_to_coeff(a_l.clone()), dom.lagrange_to_coeff(b_l.clone())
    r_c = dom.lagrange_to_coeff(dom.pointwise("mul", a_l.clone(), b_l))       # (a*b mod X^n-1), coefficients
    a_e, b_e, r_e = dom.coeff_to_extended(a_c), dom.coeff_to_extended(b_c), dom.coeff_to_extended(r_c)
    num = dom.pointwise("sub", dom.pointwise("mul", a_e, b_e), r_e)
    h_c = dom.extended_to_coeff(dom.divide_by_vanishing_poly(num))            # n*(j-1) coefficients
    torch.cuda.synchronize()
    x = 0x1234567890ABCDEF1234567890ABCDEF % p
    ev = lambda t: horner(to_ints(f, t), x, p)  # noqa: E731
    av, bv, rv, hv = ev(a_c), ev(b_c), ev(r_c), ev(h_c)
    assert (av * bv - rv - hv * (pow(x, n, p) - 1)) % p == 0
    # top half of h is zero: deg(a*b) < 2n so deg(h) < n
    assert not h_c[n:].any().item()


@pytest.mark.parametrize("curve", ["bn254", "pallas", "vesta"])
@pytest.mark.parametrize("n", [1, 2, 15, 16, 17, 1000, 1 << 12, (1 << 14) + 5, 1 << 16, (1 << 16) + 1])
def test_divide_linear_matches_kate_division(h2, curve, n):
    """h2_poly_divide_linear_device against the oracle's synthetic division (halo2_ref.pdiv_linear): every chunking
    case (one short chunk, a ragged last chunk, 4096 chunks) and q[n-1] = 0."""
    import ctypes
    import torch
    f = R.CURVES[curve].scalar
    p = f.p
    rng = R.SplitMix64(31 * n + len(curve))
    a = [R.synth_scalar(rng, p) for _ in range(n)]
    z = R.synth_scalar(rng, p)
    want, acc = [0] * n, 0
    for i in range(n - 1, 0, -1):            # pdiv_linear, written for this field (halo2_ref fixes BN254's Fr)
        acc = (a[i] + acc * z) % p
        want[i - 1] = acc
    if curve == "bn254":
        import halo2_ref as H
        assert H.pdiv_linear(a, z) == want[:n - 1]
    d_a = torch.from_numpy(np.array([f.limbs(v) for v in a], dtype=np.uint64).view(np.int64)).cuda()
    d_q = torch.full_like(d_a, -1)
    zm = np.array(f.limbs(z), dtype=np.uint64)
    L = h2.load()
    st = L.h2_poly_divide_linear_device(h2.CURVES[curve], ctypes.c_void_p(d_a.data_ptr()), n, zm.ctypes.data,
                                        ctypes.c_void_p(d_q.data_ptr()), None)
    assert st == 0
    torch.cuda.synchronize()
    assert to_ints(f, d_q) == want
    # in place is refused (the recurrence reads what a neighbour chunk writes)
    assert L.h2_poly_divide_linear_device(h2.CURVES[curve], ctypes.c_void_p(d_a.data_ptr()), n, zm.ctypes.data,
                                          ctypes.c_void_p(d_a.data_ptr()), None) == -1


def test_divide_linear_full_size_property(h2):
    """n = 2^19 (512 rows per chunk): q (X - z) + a(z) = a, checked at a random point."""
    import ctypes
    import torch
    curve, n = "pallas", 1 << 19
    cid = O.CURVE_IDS[curve]
    fid = O.CURVE_SCALAR_FIELD[cid]
    f = R.CURVES[curve].scalar
    a = O.synth_scalars(fid, 0x48324D5300000700, n).reshape(n, 4)
    z, x = 0x1234567890ABCDEF1122334455667788 % f.p, 0x0FEDCBA987654321AABBCCDDEEFF0011 % f.p
    d_a = torch.from_numpy(a.view(np.int64)).cuda()
    d_q = torch.empty_like(d_a)
    zm = np.array(f.limbs(z), dtype=np.uint64)
    assert h2.load().h2_poly_divide_linear_device(cid, ctypes.c_void_p(d_a.data_ptr()), n, zm.ctypes.data,
                                                  ctypes.c_void_p(d_q.data_ptr()), None) == 0
    torch.cuda.synchronize()
    q = d_q.cpu().numpy().view(np.uint64)
    ev = lambda col, pt: f.from_mont(O.limbs_to_int(O.eval_polynomial(fid, col, np.array(f.limbs(pt), dtype=np.uint64))))
    assert (ev(q, x) * (x - z) + ev(a, z)) % f.p == ev(a, x)
    assert not q[n - 1].any()


@pytest.mark.parametrize("curve", ["bn254", "pallas", "vesta"])
def test_chacha20_scalars_match_the_oracle_rng(h2, curve):
    """h2_chacha20_scalars_device against halo2_ref.ChaCha20Rng (rand_chacha's block function + the 512-bit
    reduction of ff's `random`).  The oracle's generator is itself pinned by the recorded proof hashes: the blinding
    polynomial it produces is committed to and opened in every proof (tests/test_proof_pins.py)."""
    import ctypes
    import torch
    import halo2_ref as H
    f = R.CURVES[curve].scalar
    seed = bytes((7 * i + 3) & 0xFF for i in range(32))
    n = 300
    rng = H.ChaCha20Rng(seed)
    want = []
    for _ in range(n):
        v = 0
        for i in range(16):
            v |= rng.next_u32() << (32 * i)
        want.append(v % f.p)
    out = torch.empty((n, 4), dtype=torch.int64, device="cuda")
    L = h2.load()
    assert L.h2_chacha20_scalars_device(h2.CURVES[curve], seed, 0, n, ctypes.c_void_p(out.data_ptr()), None) == 0
    torch.cuda.synchronize()
    assert to_ints(f, out) == want
    # a later starting block continues the same stream
    assert L.h2_chacha20_scalars_device(h2.CURVES[curve], seed, 100, 50, ctypes.c_void_p(out.data_ptr()), None) == 0
    torch.cuda.synchronize()
    assert to_ints(f, out[:50]) == want[100:150]


@pytest.mark.parametrize("curve", ["bn254", "vesta"])
@pytest.mark.parametrize("n", [1, 2, 16, 17, 1000, (1 << 14) + 3, 1 << 16, (1 << 16) + 1, 1 << 17])
def test_prefix_product_matches_the_running_product(h2, curve, n):
    """h2_poly_prefix_product_device against z[i+1] = z[i] * a[i], z[0] = 1 in big integers (zeros included: every
    later row becomes 0), out of place and in place."""
    import ctypes
    import torch
    f = R.CURVES[curve].scalar
    p = f.p
    fid = O.CURVE_SCALAR_FIELD[O.CURVE_IDS[curve]]
    a_l = O.synth_scalars(fid, 0x48324D5300000800 + n, n).reshape(n, 4).copy()
    if n > 1000:
        a_l[n - 5] = 0                                   # a vanishing ratio late in the column
    a = [f.from_mont(O.limbs_to_int(r)) for r in a_l]
    want, acc = [], 1
    for v in a:
        want.append(acc)
        acc = acc * v % p
    d_a = torch.from_numpy(a_l.view(np.int64)).cuda()
    d_o = torch.full_like(d_a, -1)
    L = h2.load()
    cid = h2.CURVES[curve]
    assert L.h2_poly_prefix_product_device(cid, ctypes.c_void_p(d_a.data_ptr()), n, ctypes.c_void_p(d_o.data_ptr()), None) == 0
    torch.cuda.synchronize()
    assert to_ints(f, d_o) == want
    assert L.h2_poly_prefix_product_device(cid, ctypes.c_void_p(d_a.data_ptr()), n, ctypes.c_void_p(d_a.data_ptr()), None) == 0
    torch.cuda.synchronize()
    assert to_ints(f, d_a) == want
