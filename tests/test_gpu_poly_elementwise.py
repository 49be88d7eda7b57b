"""GPU: the plain elementwise polynomial entry points -- h2_poly_scale_device, h2_poly_coset_device,
h2_poly_mul_periodic_device, h2_poly_pointwise_device, h2_poly_inverse_device -- against Python integers, on the scalar
fields of all three curves.  Every comparison is equality of the canonical Montgomery limbs.

Shapes: the lengths around POLY_RUN = 8 (the powers kernel's run), around one 256-thread block, one more (2049), each as
one column and as three; and one case of 2048 * 256 + 257 elements, which is poly_grid's capped grid once and a ragged
second grid-stride trip.  Data: the edge values of test_device_field_ops_match_oracle among random elements.  Every
device buffer carries GUARD elements of a sentinel behind its last element, checked after the call.
"""
import ctypes
import random

import numpy as np
import pytest

import oracle_lib as O
import pyref as R

pytestmark = pytest.mark.gpu

CURVES = ["bn254", "pallas", "vesta"]
CID = O.CURVE_IDS
EINVAL = -1
GUARD = 64
SENTINEL = np.uint64(0xA5C35A3CA5C35A3C)
SMALL_N = [1, 7, 8, 9, 255, 256, 257, 2049]
GRID_CAP = 2048 * 256                    # poly_grid: at most 2048 blocks of 256 threads
LARGE = GRID_CAP + 257
LARGE_M = 5                              # LARGE = 5 * 104909: the column count of the large case where the call takes m
assert LARGE % LARGE_M == 0
MASK64 = (1 << 64) - 1


def field(curve):
    return R.CURVES[curve].scalar


def fid(curve):
    return O.CURVE_SCALAR_FIELD[CID[curve]]


def specials(p):
    """the edge values of test_device_field_ops_match_oracle, and the two values whose STORED limbs (x 2^256 mod p) are
    the integers p - 1 and p - 2: the carry and conditional-subtraction ends of the limb arithmetic itself (the
    Montgomery form of the value p - 1 is about 2^128 on the Pasta fields)"""
    rinv = pow(1 << 256, -1, p)
    return [0, 1, 2, p - 1, p - 2, (1 << 255) % p, (1 << 32) - 1, (1 << 64) - 1, (p - 1) // 2,
            (p - 1) * rinv % p, (p - 2) * rinv % p]


def mixed(p, count, rng):
    """every third element an edge value (element 0 is p - 1), random elements between them"""
    sp = specials(p)
    return [sp[(i // 3 + 3) % len(sp)] if i % 3 == 0 else rng.randrange(p) for i in range(count)]


def ints_to_limbs(x):
    """integers below 2^256 -> (len, 4) uint64, little-endian limbs"""
    x = np.asarray(x, dtype=object).reshape(-1)
    out = np.empty((x.shape[0], 4), dtype=np.uint64)
    for j in range(4):
        out[:, j] = ((x >> (64 * j)) & MASK64).astype(np.uint64)
    return out


def limbs_to_ints(a):
    """(len, 4) uint64 -> object array of integers"""
    a = np.asarray(a, dtype=np.uint64).reshape(-1, 4)
    x = a[:, 3].astype(object)
    for j in (2, 1, 0):
        x = (x << 64) | a[:, j].astype(object)
    return x


def mont(f, vals):
    """canonical integers -> (len, 4) Montgomery limbs, the bytes the API reads and writes"""
    return ints_to_limbs([v * f.R % f.p for v in vals])


def one_elem(f, v):
    return np.array(f.limbs(v), dtype=np.uint64)


def guarded(host):
    """(rows, 4) uint64 -> device tensor of rows + GUARD elements, the guard filled with the sentinel"""
    import torch
    rows = host.shape[0]
    full = np.empty((rows + GUARD, 4), dtype=np.uint64)
    full[:rows] = host
    full[rows:] = SENTINEL
    return torch.from_numpy(full.view(np.int64)).cuda()


def fetch(buf, rows):
    """synchronise, check the guard, return the first `rows` elements"""
    import torch
    torch.cuda.synchronize()
    h = buf.cpu().numpy().view(np.uint64)
    assert h.shape[0] == rows + GUARD
    assert (h[rows:] == SENTINEL).all(), "guard behind the buffer was written"
    return h[:rows]


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


# ------------------------------------------------------------------------------ scale ----
@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("n", SMALL_N)
def test_scale_small(h2, curve, n):
    """a[i] *= c over the flattened n * m elements, c in {0, 1, p - 1, random}"""
    f = field(curve)
    p, L = f.p, h2.load()
    rng = random.Random(1000 + 7 * n + CID[curve])
    for m in (1, 3):
        vals = mixed(p, n * m, rng)
        host = mont(f, vals)
        for c in (0, 1, p - 1, rng.randrange(p)):
            buf, cm = guarded(host), one_elem(f, c)
            assert L.h2_poly_scale_device(CID[curve], ptr(buf), n, m, cm.ctypes.data, None) == 0
            assert np.array_equal(fetch(buf, n * m), mont(f, [v * c % p for v in vals])), (m, hex(c))


def large_column(curve, seed):
    """LARGE elements: random, the edge values spread over both sides of the grid wrap"""
    f = field(curve)
    a = O.synth_scalars(fid(curve), 0x48324D5300005000 + seed, LARGE).reshape(LARGE, 4).copy()
    sp = mont(f, specials(f.p))
    for j in range(len(sp)):
        for pos in (j, 1000 + 37 * j, GRID_CAP - 1 - j, GRID_CAP + j, LARGE - 1 - j):
            a[pos] = sp[(j + pos) % len(sp)]
    return a


def test_scale_grid_stride_wrap(h2):
    """2048 * 256 + 257 elements (LARGE / 5 rows x 5 columns): the capped grid and a ragged second trip"""
    curve = "bn254"
    f = field(curve)
    a = large_column(curve, 1)
    c = one_elem(f, 0x1234567890ABCDEF0FEDCBA987654321AABBCCDD % f.p)
    buf = guarded(a)
    assert h2.load().h2_poly_scale_device(CID[curve], ptr(buf), LARGE // LARGE_M, LARGE_M, c.ctypes.data, None) == 0
    want = O.field_mul_many(fid(curve), a.reshape(-1), np.tile(c, LARGE)).reshape(LARGE, 4)
    assert np.array_equal(fetch(buf, LARGE), want)


# ------------------------------------------------------------------------------ coset ----
_ZETA = {}


def coset_constants(curve, n, rng):
    from halo2_prover_amd.domain import EvaluationDomain
    f = field(curve)
    if curve not in _ZETA:
        _ZETA[curve] = EvaluationDomain(3, 4, curve).g_coset
    zeta = _ZETA[curve]
    assert zeta not in (0, 1) and pow(zeta, 3, f.p) == 1
    log_n = max(1, (n - 1).bit_length())
    return [1, f.p - 1, zeta, f.omega(log_n), rng.randrange(f.p)]


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("n", SMALL_N)
def test_coset_small(h2, curve, n):
    """a[c][i] *= g^i for i < n in every column c (stride n): every thread owns POLY_RUN = 8 consecutive i, so n = 7, 8, 9
    are a ragged run, one full run and a run of one; 2049 is a second block.  The exponent restarts at 0 in every column:
    row 0 of each column keeps its value.  g in {1, p - 1, zeta, an omega of order 2^ceil(log2 n), random}."""
    f = field(curve)
    p, L = f.p, h2.load()
    rng = random.Random(2000 + 7 * n + CID[curve])
    for m in (1, 3):
        vals = mixed(p, n * m, rng)
        host = mont(f, vals)
        for g in coset_constants(curve, n, rng):
            buf, gm = guarded(host), one_elem(f, g)
            assert L.h2_poly_coset_device(CID[curve], ptr(buf), n, m, gm.ctypes.data, None) == 0
            pw = [1] * n
            for i in range(1, n):
                pw[i] = pw[i - 1] * g % p
            got = fetch(buf, n * m)
            assert np.array_equal(got, mont(f, [vals[c * n + i] * pw[i] % p for c in range(m) for i in range(n)])), (m, hex(g))
            for c in range(m):
                assert np.array_equal(got[c * n], host[c * n]), (m, c, hex(g))     # g^0 at the head of every column


# ----------------------------------------------------------------------- mul_periodic ----
def periodic_table(p, period, rng):
    tab = [rng.randrange(p) for _ in range(period)]
    tab[0] = p - 1
    if period > 1:
        tab[1] = 0
    return tab


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("n", SMALL_N)
def test_mul_periodic_small(h2, curve, n):
    """a[i] *= t[i mod period], the index i running over the FLATTENED n * m elements: with m > 1 a column starts at
    t[(c n) mod period], which is t[0] only where the period divides n (the prover's use: period | n, a power of two).
    Periods: 1, 2, n itself where n is a power of two, and a power of two above n * m (no wrap at all); the table holds
    p - 1 and, from period 2 on, 0."""
    import torch
    f = field(curve)
    p, L = f.p, h2.load()
    rng = random.Random(3000 + 7 * n + CID[curve])
    for m in (1, 3):
        total = n * m
        vals = mixed(p, total, rng)
        host = mont(f, vals)
        periods = [1, 2, 1 << total.bit_length()]
        if (n & (n - 1)) == 0:
            periods.append(n)
        for period in periods:
            tab = periodic_table(p, period, rng)
            t_host = mont(f, tab)
            d_t = guarded(t_host)
            buf = guarded(host)
            assert L.h2_poly_mul_periodic_device(CID[curve], ptr(buf), n, m, ptr(d_t), period, None) == 0
            got = fetch(buf, total)
            assert np.array_equal(got, mont(f, [vals[i] * tab[i % period] % p for i in range(total)])), (m, period)
            if n % period == 0:      # the per-column meaning: column c, row i takes t[i mod period]
                assert np.array_equal(got, mont(f, [vals[c * n + i] * tab[i % period] % p for c in range(m) for i in range(n)]))
            assert np.array_equal(fetch(d_t, period), t_host)                       # the table is read only
            del d_t
    torch.cuda.synchronize()


def test_mul_periodic_grid_stride_wrap(h2):
    curve = "pallas"
    f = field(curve)
    a = large_column(curve, 2)
    period = 1 << 12
    t_host = O.synth_scalars(fid(curve), 0x48324D5300005100, period).reshape(period, 4).copy()
    t_host[0] = one_elem(f, f.p - 1)
    t_host[1] = 0
    d_t, buf = guarded(t_host), guarded(a)
    assert h2.load().h2_poly_mul_periodic_device(CID[curve], ptr(buf), LARGE // LARGE_M, LARGE_M, ptr(d_t), period,
                                                  None) == 0
    idx = np.arange(LARGE) % period
    want = O.field_mul_many(fid(curve), a.reshape(-1), t_host[idx].reshape(-1)).reshape(LARGE, 4)
    assert np.array_equal(fetch(buf, LARGE), want)
    assert np.array_equal(fetch(d_t, period), t_host)


# -------------------------------------------------------------------------- pointwise ----
def pointwise_want(f, op, a, b):
    """a, b: object arrays of Montgomery integers (x R mod p); the sum and the difference keep that form, the product
    needs one R taken out"""
    if op == 0:
        return (a + b) % f.p
    if op == 1:
        return (a - b) % f.p
    return a * b * f.Rinv % f.p


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("n", SMALL_N)
def test_pointwise_small(h2, curve, n):
    """a[i] = a[i] op b[i], op 0 add, 1 sub, 2 mul; then with d_b == d_a: a + a = 2a, a - a = 0, a * a = a^2"""
    f = field(curve)
    p, L = f.p, h2.load()
    rng = random.Random(4000 + 7 * n + CID[curve])
    va, vb = mixed(p, n, rng), mixed(p, n + 1, rng)[1:]           # the edge values of b sit beside those of a
    ha, hb = mont(f, va), mont(f, vb)
    d_b = guarded(hb)
    for op, fn in ((0, lambda x, y: (x + y) % p), (1, lambda x, y: (x - y) % p), (2, lambda x, y: x * y % p)):
        buf = guarded(ha)
        assert L.h2_poly_pointwise_device(CID[curve], op, ptr(buf), ptr(d_b), n, None) == 0
        assert np.array_equal(fetch(buf, n), mont(f, [fn(x, y) for x, y in zip(va, vb)])), op
        buf = guarded(ha)
        assert L.h2_poly_pointwise_device(CID[curve], op, ptr(buf), ptr(buf), n, None) == 0
        assert np.array_equal(fetch(buf, n), mont(f, [fn(x, x) for x in va])), ("aliased", op)
    assert np.array_equal(fetch(d_b, n), hb)


@pytest.mark.parametrize("curve", CURVES)
def test_pointwise_every_edge_value_against_every_edge_value(h2, curve):
    f = field(curve)
    p, L = f.p, h2.load()
    sp = specials(p)
    va = [x for x in sp for _ in sp]
    vb = [y for _ in sp for y in sp]
    n = len(va)
    d_b = guarded(mont(f, vb))
    for op, fn in ((0, lambda x, y: (x + y) % p), (1, lambda x, y: (x - y) % p), (2, lambda x, y: x * y % p)):
        buf = guarded(mont(f, va))
        assert L.h2_poly_pointwise_device(CID[curve], op, ptr(buf), ptr(d_b), n, None) == 0
        assert np.array_equal(fetch(buf, n), mont(f, [fn(x, y) for x, y in zip(va, vb)])), op


def test_pointwise_grid_stride_wrap(h2):
    """the product against the oracle's pinned multiplier, the sum and the difference against Python integers"""
    curve = "vesta"
    f = field(curve)
    a, b = large_column(curve, 3), large_column(curve, 4)[::-1].copy()
    ai, bi = limbs_to_ints(a), limbs_to_ints(b)
    d_b = guarded(b)
    L = h2.load()
    for op in (0, 1, 2):
        buf = guarded(a)
        assert L.h2_poly_pointwise_device(CID[curve], op, ptr(buf), ptr(d_b), LARGE, None) == 0
        if op == 2:
            want = O.field_mul_many(fid(curve), a.reshape(-1), b.reshape(-1)).reshape(LARGE, 4)
        else:
            want = ints_to_limbs(pointwise_want(f, op, ai, bi))
        assert np.array_equal(fetch(buf, LARGE), want), op
    assert np.array_equal(fetch(d_b, LARGE), b)


# ---------------------------------------------------------------------------- inverse ----
@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("n", SMALL_N)
def test_inverse_small(h2, curve, n):
    """a[i] = 1 / a[i], zero stays zero: the edge values as they fall (0 among them), then with zeros at 0 and n - 1"""
    f = field(curve)
    p, L = f.p, h2.load()
    rng = random.Random(5000 + 7 * n + CID[curve])
    vals = mixed(p, n, rng)
    ends = list(vals)
    ends[0] = ends[n - 1] = 0
    for col in (vals, ends):
        buf = guarded(mont(f, col))
        assert L.h2_poly_inverse_device(CID[curve], ptr(buf), n, None) == 0
        assert np.array_equal(fetch(buf, n), mont(f, [pow(x, -1, p) if x else 0 for x in col]))


def test_inverse_grid_stride_wrap(h2):
    """zeros at index 0, at the last index and on both sides of the grid wrap stay zero; every other row times its
    original is the Montgomery one -- the inverse is unique, so that is an exact check of every row"""
    curve = "vesta"
    f = field(curve)
    a = large_column(curve, 5)
    zeros = (0, GRID_CAP - 1, GRID_CAP, LARGE - 1)
    for z in zeros:
        a[z] = 0
    is_zero = ~a.any(axis=1)
    assert all(is_zero[z] for z in zeros) and is_zero.sum() < 64        # the edge value 0 among the data, too
    buf = guarded(a)
    assert h2.load().h2_poly_inverse_device(CID[curve], ptr(buf), LARGE, None) == 0
    got = fetch(buf, LARGE)
    assert not got[is_zero].any()
    prod = O.field_mul_many(fid(curve), got.reshape(-1), a.reshape(-1)).reshape(LARGE, 4)
    want = np.tile(one_elem(f, 1), (LARGE, 1))
    want[is_zero] = 0
    assert np.array_equal(prod, want)
    assert (limbs_to_ints(got) < f.p).all()                             # canonical limbs


# ---------------------------------------------------------------------------- streams ----
def test_on_a_non_default_stream(h2):
    """every entry point once on a stream of its own: the same bytes as on the default stream"""
    import torch
    curve, n, m = "pallas", 257, 3
    f = field(curve)
    p, L, cid = f.p, h2.load(), CID[curve]
    rng = random.Random(6000)
    host = mont(f, mixed(p, n * m, rng))
    other = guarded(mont(f, mixed(p, n * m, rng)))
    tab = guarded(mont(f, periodic_table(p, 256, rng)))
    c = one_elem(f, rng.randrange(p))
    calls = {
        "scale": lambda b, s: L.h2_poly_scale_device(cid, ptr(b), n, m, c.ctypes.data, s),
        "coset": lambda b, s: L.h2_poly_coset_device(cid, ptr(b), n, m, c.ctypes.data, s),
        "mul_periodic": lambda b, s: L.h2_poly_mul_periodic_device(cid, ptr(b), n, m, ptr(tab), 256, s),
        "pointwise": lambda b, s: L.h2_poly_pointwise_device(cid, 2, ptr(b), ptr(other), n * m, s),
        "inverse": lambda b, s: L.h2_poly_inverse_device(cid, ptr(b), n * m, s),
    }
    side = torch.cuda.Stream()
    for name, call in calls.items():
        buf = guarded(host)
        assert call(buf, None) == 0
        want = fetch(buf, n * m).copy()
        assert not np.array_equal(want, host), name
        buf = guarded(host)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            assert call(buf, ctypes.c_void_p(side.cuda_stream)) == 0
        side.synchronize()
        assert np.array_equal(fetch(buf, n * m), want), name


# ----------------------------------------------------------------------- status codes ----
def test_status_codes(h2):
    """n * m = 0 is H2_OK and touches nothing; a null data pointer, a null constant or table, a curve id out of range and
    a pointwise op outside 0..2 are H2_EINVAL, rejected on the host -- also when n * m = 0: the buffer keeps its
    sentinel fill"""
    import torch
    L = h2.load()
    f = field("bn254")
    fill = np.full((16, 4), SENTINEL, dtype=np.uint64)
    buf, b2 = guarded(fill), guarded(fill)
    c = one_elem(f, 5)
    cp = c.ctypes.data
    ok = []
    for n, m in ((0, 3), (5, 0), (0, 0)):
        ok += [L.h2_poly_scale_device(0, ptr(buf), n, m, cp, None), L.h2_poly_coset_device(0, ptr(buf), n, m, cp, None),
               L.h2_poly_mul_periodic_device(0, ptr(buf), n, m, ptr(b2), 4, None)]
    ok += [L.h2_poly_pointwise_device(0, op, ptr(buf), ptr(b2), 0, None) for op in (0, 1, 2)]
    ok.append(L.h2_poly_inverse_device(0, ptr(buf), 0, None))
    assert ok == [0] * len(ok)
    # the pointer, curve and period checks come before the length's: n * m = 0 does not excuse them
    first = [L.h2_poly_scale_device(0, None, 0, 3, cp, None), L.h2_poly_scale_device(0, ptr(buf), 0, 3, None, None),
             L.h2_poly_scale_device(3, ptr(buf), 0, 3, cp, None), L.h2_poly_coset_device(0, None, 5, 0, cp, None),
             L.h2_poly_coset_device(0, ptr(buf), 5, 0, None, None), L.h2_poly_coset_device(-1, ptr(buf), 0, 0, cp, None),
             L.h2_poly_mul_periodic_device(0, None, 0, 3, ptr(b2), 4, None),
             L.h2_poly_mul_periodic_device(0, ptr(buf), 0, 3, None, 4, None),
             L.h2_poly_mul_periodic_device(0, ptr(buf), 0, 3, ptr(b2), 3, None),
             L.h2_poly_mul_periodic_device(0, ptr(buf), 0, 3, ptr(b2), 0, None),
             L.h2_poly_mul_periodic_device(7, ptr(buf), 0, 3, ptr(b2), 4, None),
             L.h2_poly_pointwise_device(0, 0, None, ptr(b2), 0, None), L.h2_poly_pointwise_device(0, 0, ptr(buf), None, 0, None),
             L.h2_poly_pointwise_device(0, 3, ptr(buf), ptr(b2), 0, None),
             L.h2_poly_pointwise_device(3, 0, ptr(buf), ptr(b2), 0, None),
             L.h2_poly_inverse_device(0, None, 0, None), L.h2_poly_inverse_device(3, ptr(buf), 0, None)]
    assert first == [EINVAL] * len(first)
    bad = []
    for cid in (0, 1, 2):
        bad += [L.h2_poly_scale_device(cid, None, 4, 1, cp, None), L.h2_poly_scale_device(cid, ptr(buf), 4, 1, None, None),
                L.h2_poly_coset_device(cid, None, 4, 1, cp, None), L.h2_poly_coset_device(cid, ptr(buf), 4, 1, None, None),
                L.h2_poly_mul_periodic_device(cid, None, 4, 1, ptr(b2), 4, None),
                L.h2_poly_mul_periodic_device(cid, ptr(buf), 4, 1, None, 4, None),
                L.h2_poly_pointwise_device(cid, 0, None, ptr(b2), 4, None),
                L.h2_poly_pointwise_device(cid, 0, ptr(buf), None, 4, None),
                L.h2_poly_pointwise_device(cid, 3, ptr(buf), ptr(b2), 4, None),
                L.h2_poly_pointwise_device(cid, -1, ptr(buf), ptr(b2), 4, None),
                L.h2_poly_inverse_device(cid, None, 4, None)]
    for cid in (3, 7, -1):
        bad += [L.h2_poly_scale_device(cid, ptr(buf), 4, 1, cp, None), L.h2_poly_coset_device(cid, ptr(buf), 4, 1, cp, None),
                L.h2_poly_mul_periodic_device(cid, ptr(buf), 4, 1, ptr(b2), 4, None),
                L.h2_poly_pointwise_device(cid, 0, ptr(buf), ptr(b2), 4, None),
                L.h2_poly_inverse_device(cid, ptr(buf), 4, None)]
    assert bad == [EINVAL] * len(bad)
    assert np.array_equal(fetch(buf, 16), fill) and np.array_equal(fetch(b2, 16), fill)
    # still healthy after the refusals
    d = guarded(mont(f, [3]))
    assert L.h2_poly_scale_device(0, ptr(d), 1, 1, cp, None) == 0
    assert np.array_equal(fetch(d, 1), mont(f, [15]))
    torch.cuda.synchronize()
