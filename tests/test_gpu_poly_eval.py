"""GPU: h2_poly_eval_device / h2_poly_eval -- arithmetic.rs eval_polynomial over columns resident in HBM
(csrc/h2_poly.hpp: powers, tile and fold kernels).

The judge is Python big-integer Horner modulo the field's prime (the primes of halo2_prover_amd/domain.py).  It works
on the raw Montgomery integers: the evaluation is linear in the coefficients, so with coefficients c_i R and the true
point x the result's Montgomery integer is sum_i (c_i R) x^i mod p.  Both sides are canonical, so every comparison is
exact.  Lengths are sized by T = h2_poly_eval_tile(): the edges of a thread's run, of a tile and of the cross-tile fold."""
import ctypes
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CID = {"bn254": 0, "pallas": 1, "vesta": 2}
H2_OK, H2_EINVAL = 0, -1
PATTERN = 0x5A5A5A5A5A5A5A5A


def L():
    from halo2_prover_amd import lib
    return lib.load()


def tile():
    return L().h2_poly_eval_tile()


def prime(curve):
    from halo2_prover_amd.domain import _FIELDS
    return _FIELDS[CID[curve]][0]


def root_of_unity(curve, k):
    """a primitive 2^k-th root of unity"""
    from halo2_prover_amd.domain import _FIELDS
    p, gen, S, _ = _FIELDS[CID[curve]]
    return pow(pow(gen, (p - 1) >> S, p), 1 << (S - k), p)


def raw_limbs(values):
    """ints below 2^256 -> (len, 4) uint64"""
    buf = b"".join(v.to_bytes(32, "little") for v in values)
    return np.frombuffer(buf, dtype=np.uint64).reshape(-1, 4).copy()


def raw_ints(a):
    buf = np.ascontiguousarray(a).tobytes()
    return [int.from_bytes(buf[i:i + 32], "little") for i in range(0, len(buf), 32)]


def mont_points(curve, points):
    p = prime(curve)
    R = (1 << 256) % p
    return raw_limbs([x % p * R % p for x in points]).reshape(-1)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).cuda()


def horner(coeffs, x, p):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % p
    return acc


def call(curve, ptrs, n, points, d_out, stream=None):
    """points: true values; ptrs: device addresses"""
    q = len(ptrs)
    arr = (ctypes.c_void_p * max(q, 1))(*ptrs)
    pm = mont_points(curve, points) if q else np.zeros(4, dtype=np.uint64)
    return L().h2_poly_eval_device(CID[curve], arr, n, pm.ctypes.data, q, ctypes.c_void_p(d_out.data_ptr()), stream)


def evaluate(curve, cols, jobs, stream=None):
    """cols: list of (n, 4) device tensors; jobs: (column index, point) pairs -> raw result integers"""
    import torch
    n = cols[0].shape[0]
    out = torch.full((len(jobs), 4), PATTERN, dtype=torch.int64, device="cuda")
    st = call(curve, [cols[c].data_ptr() for c, _ in jobs], n, [x for _, x in jobs], out, stream)
    assert st == H2_OK
    torch.cuda.synchronize()
    return raw_ints(out.cpu().numpy().view(np.uint64))


def random_raw(p, rng, n):
    return [rng.randrange(p) for _ in range(n)]


# name -> (multiple of T, offset)
LENGTHS = {"0": (0, 0), "1": (0, 1), "2": (0, 2), "3": (0, 3), "7": (0, 7), "8": (0, 8), "9": (0, 9), "T-1": (1, -1),
           "T": (1, 0), "T+1": (1, 1), "2T+3": (2, 3), "5T-1": (5, -1)}


def length_of(tag, T):
    mult, off = LENGTHS[tag]
    return mult * T + off


@pytest.mark.parametrize("tag", list(LENGTHS))
@pytest.mark.parametrize("curve", ["bn254", "pallas", "vesta"])
def test_lengths_columns_and_points(h2, curve, tag):
    p = prime(curve)
    n = length_of(tag, tile())
    rng = random.Random(0x9E3779B9 ^ (n * 3 + CID[curve]))
    R = (1 << 256) % p
    # raw Montgomery integers: random canonical, all p - 1 (the largest integer the lazy form must carry), all zero,
    # and the field's one
    columns = [random_raw(p, rng, n), [p - 1] * n, [0] * n, [R] * n]
    k = max(n - 1, 0).bit_length()
    omega = root_of_unity(curve, k)
    points = [0, 1, p - 1, 2, rng.randrange(p), omega]
    # every column at every point in ONE call: a column at several points, a point on several columns
    jobs = [(c, x) for c in range(len(columns)) for x in points]
    cols = [dev(raw_limbs(col).reshape(n, 4)) for col in columns]
    got = evaluate(curve, cols, jobs)
    want = [horner(columns[c], x, p) for c, x in jobs]
    assert got == want
    if n > 1 and n & (n - 1) == 0:
        assert got[jobs.index((3, omega))] == 0          # 1 + w + ... + w^(n-1) = 0
    if n:
        assert got[jobs.index((0, 0))] == columns[0][0]  # 0^0 = 1: a zero point returns coefficient 0
    else:
        assert got == [0] * len(jobs)


def test_one_real_size(h2):
    """n = 2^16, 32 distinct random jobs on BN254"""
    p = prime("bn254")
    n, q = 1 << 16, 32
    rng = np.random.default_rng(0x48324556)
    a = rng.integers(0, 1 << 64, size=(q, n, 4), dtype=np.uint64)
    a[..., 3] = rng.integers(0, p >> 192, size=(q, n), dtype=np.uint64)      # below p: canonical
    prng = random.Random(0x48324557)
    points = [prng.randrange(p) for _ in range(q)]
    d = dev(a)
    got = evaluate("bn254", [d[j] for j in range(q)], list(enumerate(points)))
    want = [horner(raw_ints(a[j]), points[j], p) for j in range(q)]
    assert got == want


@pytest.mark.parametrize("q", [1, 33, 70000])
def test_job_counts(h2, q):
    """d_polys cycles over 3 columns; 70 000 jobs cross the grid.y limit and the grouping"""
    curve, n = "pallas", 4
    p = prime(curve)
    rng = random.Random(1000 + q)
    columns = [random_raw(p, rng, n) for _ in range(3)]
    cols = [dev(raw_limbs(col)) for col in columns]
    jobs = [(t % 3, rng.randrange(p)) for t in range(q)]
    got = evaluate(curve, cols, jobs)
    assert got == [horner(columns[c], x, p) for c, x in jobs]


def test_no_jobs_enqueue_nothing(h2):
    import torch
    out = torch.full((4, 4), PATTERN, dtype=torch.int64, device="cuda")
    col = dev(raw_limbs([1, 2, 3, 4]))
    assert call("bn254", [], 4, [], out) == H2_OK
    assert L().h2_poly_eval_device(0, None, 4, None, 0, None, None) == H2_OK
    torch.cuda.synchronize()
    assert bool((out == PATTERN).all())
    del col


def test_streams_agree(h2):
    import torch
    curve = "vesta"
    p = prime(curve)
    n = tile() + 5
    rng = random.Random(77)
    columns = [random_raw(p, rng, n) for _ in range(2)]
    cols = [dev(raw_limbs(col)) for col in columns]
    jobs = [(0, rng.randrange(p)), (1, rng.randrange(p)), (0, 3)]
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        on_stream = evaluate(curve, cols, jobs, ctypes.c_void_p(s.cuda_stream))
    on_null = evaluate(curve, cols, jobs, None)
    assert on_stream == on_null == [horner(columns[c], x, p) for c, x in jobs]


@pytest.mark.parametrize("curve", ["bn254", "pallas", "vesta"])
def test_host_form_agrees(h2, curve):
    p = prime(curve)
    n = 2 * tile() + 3
    rng = random.Random(5 + CID[curve])
    col = random_raw(p, rng, n)
    x = rng.randrange(p)
    a = raw_limbs(col)
    xm = mont_points(curve, [x])
    out = np.full(4, PATTERN, dtype=np.uint64)
    assert L().h2_poly_eval(CID[curve], a.ctypes.data, n, xm.ctypes.data, out.ctypes.data) == H2_OK
    want = horner(col, x, p)
    assert raw_ints(out) == [want]
    assert evaluate(curve, [dev(a)], [(0, x)]) == [want]
    zero = np.full(4, PATTERN, dtype=np.uint64)
    assert L().h2_poly_eval(CID[curve], None, 0, xm.ctypes.data, zero.ctypes.data) == H2_OK
    assert raw_ints(zero) == [0]


def test_invalid_arguments(h2):
    import torch
    curve = "bn254"
    p = prime(curve)
    n = 9
    rng = random.Random(99)
    col = random_raw(p, rng, n + 1)
    d = dev(raw_limbs(col))                    # n + 1 elements: d + 8 bytes still has n elements behind it
    out = torch.full((1, 4), PATTERN, dtype=torch.int64, device="cuda")
    x = rng.randrange(p)
    want = [horner(col[:n], x, p)]
    one = (ctypes.c_void_p * 1)(d.data_ptr())
    xm = mont_points(curve, [x])
    o = ctypes.c_void_p(out.data_ptr())
    f = L().h2_poly_eval_device

    def still_right():
        assert evaluate(curve, [d[:n]], [(0, x)]) == want

    still_right()
    assert f(7, one, n, xm.ctypes.data, 1, o, None) == H2_EINVAL                 # unknown curve
    still_right()
    assert f(0, None, n, xm.ctypes.data, 1, o, None) == H2_EINVAL                # null arrays with q > 0
    still_right()
    assert f(0, one, n, None, 1, o, None) == H2_EINVAL
    still_right()
    assert f(0, one, n, xm.ctypes.data, 1, None, None) == H2_EINVAL
    still_right()
    null = (ctypes.c_void_p * 1)(None)
    assert f(0, null, n, xm.ctypes.data, 1, o, None) == H2_EINVAL                # a null polynomial
    still_right()
    odd = (ctypes.c_void_p * 1)(d.data_ptr() + 8)
    assert f(0, odd, n, xm.ctypes.data, 1, o, None) == H2_EINVAL                 # 8- but not 16-byte aligned
    still_right()
    assert f(0, one, (1 << 30) + 1, xm.ctypes.data, 1, o, None) == H2_EINVAL     # checked before any access
    still_right()
    torch.cuda.synchronize()
    assert bool((out == PATTERN).all())                                          # no refused call wrote anything


def test_python_layer(h2):
    import torch
    from halo2_prover_amd.domain import EvaluationDomain
    dom = EvaluationDomain(3, 4, "bn254")
    p = dom.p
    n = tile() + 77
    rng = random.Random(4242)
    R = dom.R
    true_cols = [[rng.randrange(p) for _ in range(n)] for _ in range(3)]
    cols = dev(np.stack([raw_limbs([v * R % p for v in col]) for col in true_cols]))      # (3, n, 4)
    pts = [rng.randrange(p) for _ in range(3)]
    assert dom.eval_polynomial(cols, pts) == [horner(true_cols[j], pts[j], p) for j in range(3)]
    assert dom.eval_polynomial(cols, pts[0]) == [horner(true_cols[j], pts[0], p) for j in range(3)]
    # the same values through the C call
    raw = evaluate("bn254", [cols[j] for j in range(3)], list(enumerate(pts)))
    rinv = pow(R, -1, p)
    assert [v * rinv % p for v in raw] == dom.eval_polynomial(cols, pts)
    # kate_division: a(r) - a(z) = q(r) (r - z), the three values through the new call
    a = cols[0].contiguous()
    z, r = rng.randrange(p), rng.randrange(p)
    qcol = torch.empty_like(a)
    zm = mont_points("bn254", [z])
    st = L().h2_poly_divide_linear_device(0, ctypes.c_void_p(a.data_ptr()), n, zm.ctypes.data, ctypes.c_void_p(qcol.data_ptr()),
                                          None)
    assert st == H2_OK
    torch.cuda.synchronize()
    a_r, a_z, q_r = dom.eval_polynomial(torch.stack([a, a, qcol]), [r, z, r])
    assert (a_r - a_z) % p == q_r * (r - z) % p
    assert a_z == horner(true_cols[0], z, p)
