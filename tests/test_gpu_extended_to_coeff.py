"""GPU: h2_extended_to_coeff_device -- EvaluationDomain::extended_to_coeff (with divide_by_vanishing_poly before it when
a t table is given) as one call: the t factor on the first NTT pass's load, the zeta^-j factor, the 1 / 2^ext_k scale and
the truncation on the last pass's exit (csrc/h2_ntt29.hpp, the dividing pass 0 and the shrinking final pass).

Two judges, neither of them the code under test:
  (a) big integers, for ext_log_n <= 8: the scaled inverse DFT with the t factor and zeta^-j, in Python ints;
  (b) the composed route on entry points that other tests pin: a clone of the source, h2_poly_mul_periodic_device (when
      t is given), h2_ntt_scaled_device, h2_poly_coset_device with zeta^-1, the slice.  Both routes promise canonical
      output, so the comparison is byte for byte.  zeta is the domain's real coset generator (zeta^3 = 1), so that g^i
      and zi[i mod 3] agree.
  (c) round trip: h2_coeff_to_extended_device of n random coefficients, then the new call with out_len > n, returns the
      coefficients followed by zeros.
ext_log_n values are those at which a branch of the plan or of the kernel can go wrong: a single element; tiles under 8
rows (the non-fused load and exit); an odd and an even radix; a mid-size and the largest one-pass plan (both variants in
one launch); two passes 6 + 5 (the scale in the table); the prover's 10 + 9 with two tile columns; 10 + 10; three
passes.  At each: out_len in {2^e, 7/8, 3/4, 1/2 + 1, 5, 1} and t_period in {none, 1, 8, 2^e} where legal and distinct.
The composed reference is computed once per (shape, t) and sliced for every out_len."""
import ctypes

import numpy as np
import pytest

import pyref as R

pytestmark = pytest.mark.gpu

CID = {"bn254": 0, "pallas": 1, "vesta": 2}
H2_OK, H2_EINVAL = 0, -1
FILL = 0x5A5A5A5A5A5A5A5A

EXT_LOGS = [0, 1, 2, 3, 4, 7, 10, 11, 19, 20, 21]
OTHER_CURVE_LOGS = [6, 11, 19]
CASES = [("bn254", e) for e in EXT_LOGS] + [(c, e) for c in ("pallas", "vesta") for e in OTHER_CURVE_LOGS]
EXTRA = [(c, e) for c in ("bn254", "pallas", "vesta") for e in OTHER_CURVE_LOGS]
SMALL = [(c, e) for c, e in CASES if e <= 8]


def _ids(cases):
    return ["%s-%d" % (c, e) for c, e in cases]


def field(curve):
    return R.CURVES[curve].scalar


def zeta_of(curve):
    """the cube root of unity EvaluationDomain uses as its coset generator"""
    from halo2_prover_amd.domain import _FIELDS
    p, gen, _, zeta = _FIELDS[CID[curve]]
    z = zeta if zeta is not None else pow(gen, (p - 1) // 3, p)
    assert z != 1 and pow(z, 3, p) == 1
    return z


def constants(curve, e):
    """(ext_omega_inv, scale = 1 / 2^e, zeta_inv) as canonical ints"""
    f = field(curve)
    return pow(f.omega(e), -1, f.p), pow(1 << e, -1, f.p), pow(zeta_of(curve), 2, f.p)


def limbs_arr(f, x):
    return np.array(f.limbs(x), dtype=np.uint64)


def int_to_raw(v):
    return [(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)]


def random_columns(p, seed, rows, count):
    """(rows, count, 4) uint64: uniformly random limbs with the top limb below p's, so every element is canonical
    (any value below p is the Montgomery form of some field element)"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 1 << 64, size=(rows, count, 4), dtype=np.uint64)
    a[..., 3] = rng.integers(0, p >> 192, size=(rows, count), dtype=np.uint64)
    return a


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).cuda()


def ptr_of(x):
    """a tensor's address, an int taken as an address, or NULL"""
    if x is None:
        return None
    return ctypes.c_void_p(x if isinstance(x, int) else x.data_ptr())


def out_lens(e):
    en = 1 << e
    seen = []
    for v in (en, 7 * en // 8, 3 * en // 4, en // 2 + 1, 5, 1):
        if 1 <= v <= en and v not in seen:
            seen.append(v)
    return seen


def t_periods(e):
    seen = [None]
    for v in (1, 8, 1 << e):
        v = min(v, 1 << e)
        if v not in seen:
            seen.append(v)
    return seen


def t_table(curve, e, period, seed=0):
    """`period` random canonical elements on the device (None: no table)"""
    if period is None:
        return None
    return dev(random_columns(field(curve).p, 21000 + 37 * e + period % 1009 + CID[curve] + seed, 1, period))[0]


def fused(curve, src, e, m, t, period, out, out_len, out_stride, stream=None, cid=None, omega_inv=True, scale=True,
          zeta_inv=True):
    from halo2_prover_amd import lib
    f = field(curve)
    wi, sc, zi = (limbs_arr(f, v) for v in constants(curve, min(e, 28)))
    return lib.load().h2_extended_to_coeff_device(
        CID[curve] if cid is None else cid, ptr_of(src), e, m, wi.ctypes.data if omega_inv else None,
        sc.ctypes.data if scale else None, zi.ctypes.data if zeta_inv else None, ptr_of(t), period or 0, ptr_of(out), out_len,
        out_stride, stream)


def composed(curve, cols, e, t, period):
    """cols: (m, 2^e, 4) device tensor -> the full (m, 2^e, 4) coefficient columns, zeta^-j applied, through a clone:
    h2_poly_mul_periodic_device (when t is given), h2_ntt_scaled_device, h2_poly_coset_device"""
    from halo2_prover_amd import lib
    L = lib.load()
    f = field(curve)
    m, en = cols.shape[0], 1 << e
    a = cols.clone()
    wi, sc, zi = (limbs_arr(f, v) for v in constants(curve, e))
    ptr = ctypes.c_void_p(a.data_ptr())
    if t is not None:
        lib.check(L.h2_poly_mul_periodic_device(CID[curve], ptr, en, m, ctypes.c_void_p(t.data_ptr()), period, None),
                  "h2_poly_mul_periodic_device")
    lib.check(L.h2_ntt_scaled_device(CID[curve], ptr, m, wi.ctypes.data, e, sc.ctypes.data, None), "h2_ntt_scaled_device")
    lib.check(L.h2_poly_coset_device(CID[curve], ptr, en, m, zi.ctypes.data, None), "h2_poly_coset_device")
    return a


def run_fused(curve, cols, e, t, period, out_len, stream=None):
    import torch
    from halo2_prover_amd import lib
    m = cols.shape[0]
    out = torch.full((m, out_len, 4), FILL, dtype=torch.int64, device="cuda")
    lib.check(fused(curve, cols, e, m, t, period, out, out_len, out_len, stream), "h2_extended_to_coeff_device")
    return out


def to_ints(f, t):
    a = t.cpu().numpy().view(np.uint64).reshape(-1, 4)
    return [f.from_mont(sum(int(x) << (64 * i) for i, x in enumerate(r))) for r in a]


def bigint_coeffs(curve, ext, e, t):
    """out[j] = zi^(j mod 3) * scale * sum_i ext[i] * t[i mod period] * ext_omega_inv^(i j), all 2^e of them"""
    p = field(curve).p
    wi, sc, zi = constants(curve, e)
    en = 1 << e
    x = [v * (t[i % len(t)] if t else 1) % p for i, v in enumerate(ext)]
    pw = [pow(wi, i, p) for i in range(en)]
    return [pow(zi, j % 3, p) * sc * sum(x[i] * pw[(i * j) % en] for i in range(en)) % p for j in range(en)]


@pytest.mark.parametrize("curve,e", SMALL, ids=_ids(SMALL))
def test_against_big_integers(h2, curve, e):
    import torch
    f = field(curve)
    cols = dev(random_columns(f.p, 7000 + e + CID[curve], 2, 1 << e))
    keep = cols.clone()
    for period in t_periods(e):
        t = t_table(curve, e, period)
        want = [bigint_coeffs(curve, to_ints(f, cols[c]), e, to_ints(f, t) if t is not None else None) for c in range(2)]
        for out_len in out_lens(e):
            got = run_fused(curve, cols, e, t, period, out_len)
            torch.cuda.synchronize()
            for c in range(2):
                assert to_ints(f, got[c]) == want[c][:out_len], (period, out_len, c)
    assert torch.equal(cols, keep)


@pytest.mark.parametrize("curve,e", CASES, ids=_ids(CASES))
def test_equals_the_composed_route(h2, curve, e):
    import torch
    f = field(curve)
    cols = dev(random_columns(f.p, 9000 + e + CID[curve], 2, 1 << e))
    keep = cols.clone()
    for period in t_periods(e):
        t = t_table(curve, e, period)
        want = composed(curve, cols, e, t, period)
        for out_len in out_lens(e):
            got = run_fused(curve, cols, e, t, period, out_len)
            torch.cuda.synchronize()
            assert torch.equal(got, want[:, :out_len, :]), (period, out_len)
    assert torch.equal(cols, keep)


ROUND_TRIPS = [("bn254", 0, 1), ("bn254", 3, 6), ("bn254", 8, 11), ("bn254", 16, 19), ("pallas", 8, 11), ("vesta", 8, 11)]


@pytest.mark.parametrize("curve,log_n,e", ROUND_TRIPS, ids=["%s-%d-%d" % c for c in ROUND_TRIPS])
def test_round_trip_through_coeff_to_extended(h2, curve, log_n, e):
    """coefficients -> coset evaluations -> coefficients: the n coefficients come back, followed by zeros"""
    import torch
    from halo2_prover_amd import lib
    f = field(curve)
    n, en, m = 1 << log_n, 1 << e, 2
    coeffs = dev(random_columns(f.p, 10000 + e + CID[curve], m, n))
    ext = torch.empty((m, en, 4), dtype=torch.int64, device="cuda")
    z, w = limbs_arr(f, zeta_of(curve)), limbs_arr(f, f.omega(e))
    lib.check(lib.load().h2_coeff_to_extended_device(CID[curve], ctypes.c_void_p(coeffs.data_ptr()), n, log_n, m, z.ctypes.data,
                                                     w.ctypes.data, e, ctypes.c_void_p(ext.data_ptr()), None),
              "h2_coeff_to_extended_device")
    out_len = max(3 * en // 4, n + 1)
    got = run_fused(curve, ext, e, None, None, out_len)
    torch.cuda.synchronize()
    assert torch.equal(got[:, :n, :], coeffs)
    assert not got[:, n:, :].any().item()


@pytest.mark.parametrize("curve,e", EXTRA, ids=_ids(EXTRA))
def test_strided_destination_keeps_its_slack(h2, curve, e):
    """m = 3, out_stride = out_len + 5, the destination pre-filled: the five slack rows of every column and everything
    behind the last column keep the fill -- the truncation never stores at or beyond out_len; the source is bit-identical
    afterwards"""
    import torch
    from halo2_prover_amd import lib
    f = field(curve)
    en, m = 1 << e, 3
    cols = dev(random_columns(f.p, 11000 + e + CID[curve], m, en))
    keep = cols.clone()
    for period in (None, min(8, en)):
        t = t_table(curve, e, period)
        want = composed(curve, cols, e, t, period)
        for out_len in (3 * en // 4, en // 2 + 1):
            stride = out_len + 5
            out = torch.full((m * stride + 7, 4), FILL, dtype=torch.int64, device="cuda")
            lib.check(fused(curve, cols, e, m, t, period, out, out_len, stride), "h2_extended_to_coeff_device")
            torch.cuda.synchronize()
            body = out[: m * stride].reshape(m, stride, 4)
            assert torch.equal(body[:, :out_len, :], want[:, :out_len, :]), (period, out_len)
            assert (body[:, out_len:, :] == FILL).all().item(), (period, out_len)
            assert (out[m * stride:] == FILL).all().item(), (period, out_len)
    assert torch.equal(cols, keep)


@pytest.mark.parametrize("curve,e", EXTRA, ids=_ids(EXTRA))
def test_on_a_non_default_stream(h2, curve, e):
    import torch
    f = field(curve)
    en = 1 << e
    cols = dev(random_columns(f.p, 13000 + e + CID[curve], 2, en))
    t = t_table(curve, e, 8)
    want = composed(curve, cols, e, t, 8)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        got = run_fused(curve, cols, e, t, 8, 3 * en // 4, ctypes.c_void_p(s.cuda_stream))
    s.synchronize()
    assert torch.equal(got, want[:, : 3 * en // 4, :])


@pytest.mark.parametrize("curve,e", EXTRA, ids=_ids(EXTRA))
def test_magnitude_extremes(h2, curve, e):
    """stored values at the ends of the canonical range: a column of p - 1, a column of zeros (the output is all zero)
    and a random column holding 0, 1 and p - 1, with t entries of p - 1 and 1 (the pass's magnitude bound is written for
    canonical inputs and products in (-p, p/128])"""
    import torch
    f = field(curve)
    en, p = 1 << e, f.p
    host = random_columns(p, 15000 + e + CID[curve], 3, en)
    host[0, :, :] = np.array(int_to_raw(p - 1), dtype=np.uint64)
    host[1, :, :] = 0
    for pos, v in ((0, 0), (1, 1), (2, p - 1), (en - 3, p - 1), (en - 2, 1), (en - 1, 0)):
        host[2, pos, :] = np.array(int_to_raw(v), dtype=np.uint64)
    cols = dev(host)
    th = random_columns(p, 16000 + e + CID[curve], 1, 8)[0]
    th[0, :] = np.array(int_to_raw(p - 1), dtype=np.uint64)          # the largest canonical bytes
    th[1, :] = np.array(int_to_raw(f.to_mont(1)), dtype=np.uint64)
    th[2, :] = np.array(int_to_raw(f.to_mont(p - 1)), dtype=np.uint64)
    th[3, :] = np.array(int_to_raw(1), dtype=np.uint64)
    t = dev(th)
    for tt, period in ((None, None), (t, 8)):
        want = composed(curve, cols, e, tt, period)
        for out_len in (en, 3 * en // 4):
            got = run_fused(curve, cols, e, tt, period, out_len)
            torch.cuda.synchronize()
            assert torch.equal(got, want[:, :out_len, :]), (period, out_len)
            assert not got[1].any().item()
    if e <= 8:
        got = run_fused(curve, cols, e, t, 8, en)
        for c in range(3):
            assert to_ints(f, got[c]) == bigint_coeffs(curve, to_ints(f, cols[c]), e, to_ints(f, t))


def test_status_codes(h2):
    """every H2_EINVAL of the header, rejected on the host: nothing is enqueued, so source and destination are unchanged"""
    import torch
    curve, e = "bn254", 6
    f = field(curve)
    en, m, out_len = 1 << e, 2, 48
    # one allocation, so that overlapping ranges can be built on purpose: [ source m * en | destination m * out_len | t 8 ]
    buf = torch.full((m * en + m * out_len + 8, 4), FILL, dtype=torch.int64, device="cuda")
    buf[: m * en] = dev(random_columns(f.p, 17000, m, en)).reshape(m * en, 4)
    buf[m * en + m * out_len:] = t_table(curve, e, 8)
    src, out, t = buf[: m * en], buf[m * en: m * en + m * out_len], buf[m * en + m * out_len:]
    keep = buf.clone()
    torch.cuda.synchronize()
    ok = dict(curve=curve, src=src, e=e, m=m, t=t, period=8, out=out, out_len=out_len, out_stride=out_len)

    def call(**kw):
        a = dict(ok)
        a.update(kw)
        return fused(**a)

    bad = [
        call(cid=7),                                                    # unknown curve
        call(src=None), call(out=None),                                 # null device pointers
        call(omega_inv=False), call(scale=False), call(zeta_inv=False),  # null constants
        call(e=31, out=buf),                                            # above h2_ntt_scaled_device's limit
        call(out_len=en + 1, out_stride=en + 1),                        # out_len > 2^ext_log_n
        call(out_stride=out_len - 1),                                   # out_stride < out_len
        call(m=65536),                                                  # grid.y
        call(period=0), call(period=3), call(period=2 * en),            # t_period: zero, no power of two, too long
        call(src=src.data_ptr() + 8), call(out=out.data_ptr() + 8), call(t=t.data_ptr() + 8),    # not 16-byte aligned
        call(out=src),                                                  # destination = source
        call(out=buf[m * en - 1:]),                                     # last source element overlapped
        call(src=buf[m * out_len - 1:], out=buf, t=None),               # first source element overlapped
    ]
    torch.cuda.synchronize()
    assert bad == [H2_EINVAL] * len(bad)
    assert torch.equal(buf, keep)
    # m = 0 and out_len = 0: fine, whatever the pointers, and nothing happens
    assert call(m=0) == H2_OK
    assert call(m=0, src=None, out=None, omega_inv=False, scale=False, zeta_inv=False) == H2_OK
    assert call(out_len=0, out_stride=0) == H2_OK
    assert call(out_len=0, out_stride=0, src=None, out=None, omega_inv=False, scale=False, zeta_inv=False) == H2_OK
    torch.cuda.synchronize()
    assert torch.equal(buf, keep)
    # adjacent ranges do not overlap; without a table t_period is ignored
    assert call() == H2_OK
    torch.cuda.synchronize()
    want = composed(curve, src.reshape(m, en, 4), e, t, 8)
    assert torch.equal(out.reshape(m, out_len, 4), want[:, :out_len, :])
    assert torch.equal(src, keep[: m * en])
    assert call(t=None, period=3) == H2_OK
    torch.cuda.synchronize()
    assert torch.equal(out.reshape(m, out_len, 4), composed(curve, src.reshape(m, en, 4), e, None, None)[:, :out_len, :])


DOMAINS = [(4, 5), (5, 10), (3, 4)]


@pytest.mark.parametrize("j,k", DOMAINS, ids=["j%d-k%d" % d for d in DOMAINS])
def test_domain_level(h2, j, k):
    """EvaluationDomain: extended_to_coeff(coeff_to_extended(c)) is c padded with zeros; with divide_by_vanishing=True
    it equals the composed pair on a clone; the argument is unchanged by the call"""
    import torch
    from halo2_prover_amd import lib
    from halo2_prover_amd.domain import EvaluationDomain
    dom = EvaluationDomain(j, k)
    n, en, hlen = dom.n, 1 << dom.extended_k, dom.n * (j - 1)
    c = dev(random_columns(dom.p, 19000 + k, 2, n))
    back = dom.extended_to_coeff(dom.coeff_to_extended(c))
    torch.cuda.synchronize()
    assert back.shape == (2, hlen, 4)
    assert torch.equal(back[:, :n, :], c) and not back[:, n:, :].any().item()
    x = dev(random_columns(dom.p, 19500 + k, 2, en))
    keep = x.clone()
    got = dom.extended_to_coeff(x, divide_by_vanishing=True)
    torch.cuda.synchronize()
    assert torch.equal(x, keep)
    # the composed pair, on a clone: divide_by_vanishing_poly, then ifft, un-shift and slice by hand
    y = dom.divide_by_vanishing_poly(x.clone())
    ptr = ctypes.c_void_p(y.data_ptr())
    L = lib.load()
    lib.check(L.h2_ntt_scaled_device(dom.curve, ptr, 2, dom._m["extended_omega_inv"].ctypes.data, dom.extended_k,
                                     dom._m["extended_ifft_divisor"].ctypes.data, None), "h2_ntt_scaled_device")
    lib.check(L.h2_poly_coset_device(dom.curve, ptr, en, 2, dom._m["g_coset_inv"].ctypes.data, None), "h2_poly_coset_device")
    torch.cuda.synchronize()
    assert got.shape == (2, hlen, 4)
    assert torch.equal(got, y[:, :hlen, :])
