"""GPU: the two kernels built from the single-chain product (csrc/h2_field29_chain.hpp) against the CPU oracle.

* msm_chunk_kernel (xyzz29_add_affine<CV, Fe29Chain>), Pallas and Vesta: n = 1, 2, 63, 64, 65, 257, 4096 with one
  column, and three columns of one launch against per-column tables (h2_msm_device_multi).  The columns hold repeated
  points with equal scalars (the doubling branch inside the new instantiation) and with opposite scalars, a point beside
  its negative with one scalar (the identity branch), an all-zero column and an all-equal column.  Group elements:
  compared after affine normalisation.
* the NTT pass (radix4, emit and load_el of every instantiation), both Pasta scalar fields, forward and inverse-scaled,
  bytewise: log n = 1..4 (the unfused tile, a radix-2 and a radix-4 first stage), 9 and 10 (one pass, odd and even
  radix), 11 (two passes, a small second radix), 16 (two passes, twiddles in LDS), 19 (two passes, the 1024-row tile
  with its twiddles in global memory; one column).  One call each of h2_coeff_to_extended_device and
  h2_extended_to_coeff_device at (k, extended k) = (8, 11): the extending, dividing and shrinking instantiations.
"""
import ctypes

import numpy as np
import pytest

import oracle_lib as O
import pyref as R

pytestmark = pytest.mark.gpu

PASTA_CURVES = ["pallas", "vesta"]
CID = O.CURVE_IDS
SEED = 0x48324D5300C4A100


def scalar_field(curve):
    return R.CURVES[curve].scalar


def fid_of(curve):
    return O.CURVE_SCALAR_FIELD[CID[curve]]


def limbs_arr(f, x):
    return np.array(f.limbs(x), dtype=np.uint64)


def norm(curve, jac):
    return O.to_affine(CID[curve], np.asarray(jac, dtype=np.uint64).reshape(-1))


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).cuda()


# ------------------------------------------------------------------------------- MSM ----
def msm_inputs(curve, n):
    """(bases A, bases B, three columns): A and B repeat a point; column 0 gives the repeats equal scalars (P + P in one
    bucket: the doubling branch) and opposite ones, and a point beside its negative one scalar (P - P in one bucket: the
    identity branch); column 1 is zero, column 2 is one value on every row"""
    f = scalar_field(curve)
    ba = O.synth_bases(CID[curve], SEED | 0xA, n).reshape(n, 8)
    bb = O.synth_bases(CID[curve], SEED | 0xB, n).reshape(n, 8)
    col = O.synth_scalars(fid_of(curve), SEED | (n & 0xFF), n).reshape(n, 4)
    if n >= 2:
        ba[1] = ba[0]
        bb[1] = bb[0]
        col[1] = col[0]                                        # s P + s P
    if n >= 63:
        ba[3] = ba[2]
        s = f.from_mont(O.limbs_to_int(col[2]))
        col[3] = limbs_arr(f, (-s) % f.p)                      # s P - s P
        c = R.CURVES[curve]                                    # and -Q beside Q with one scalar: Q - Q inside one bucket
        neg = ba[4].copy()
        y = c.base.from_mont(O.limbs_to_int(neg[4:]))
        neg[4:] = np.array(c.base.limbs((-y) % c.base.p), dtype=np.uint64)
        ba[5] = neg
        col[5] = col[4]
        ba[40:44] = ba[40]                                     # a run of one point, random scalars
    zero = np.zeros((n, 4), dtype=np.uint64)
    equal = np.tile(limbs_arr(f, 0x1234567 << 17), (n, 1))
    return ba, bb, [col, zero, equal]


@pytest.mark.parametrize("curve", PASTA_CURVES)
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 257, 4096])
def test_msm_through_the_chain_accumulate_kernel(h2, curve, n):
    import torch
    from halo2_prover_amd import api
    cid = CID[curve]
    ba, bb, cols = msm_inputs(curve, n)
    A, B = h2.Bases(curve, ba), h2.Bases(curve, bb)
    try:
        # m = 1
        want0 = norm(curve, O.best_multiexp(cid, cols[0], ba, threads=4))
        got0 = norm(curve, A.msm(cols[0]))
        assert np.array_equal(got0, want0)
        assert O.is_on_curve(cid, got0)
        # m = 3, per-column tables
        which = [A, B, B]
        d = dev(np.stack(cols))
        out = torch.zeros((3, 12), dtype=torch.int64, device="cuda")
        api.msm_device_multi(which, d.data_ptr(), 0, n, n, out.data_ptr())
        torch.cuda.synchronize()
        res = out.cpu().numpy().view(np.uint64)
        assert np.array_equal(norm(curve, res[0]), want0)
        assert not norm(curve, res[1]).any()                   # the zero column: the identity
        assert np.array_equal(norm(curve, res[2]), norm(curve, O.best_multiexp(cid, cols[2], bb, threads=4)))
    finally:
        A.release()
        B.release()


# ------------------------------------------------------------------------------- NTT ----
@pytest.mark.parametrize("curve", PASTA_CURVES)
@pytest.mark.parametrize("log_n", [1, 2, 3, 4, 9, 10, 11, 16, 19])
def test_ntt_forward_and_inverse_scaled_bytewise(h2, curve, log_n):
    import torch
    f, fid = scalar_field(curve), fid_of(curve)
    L = h2.load()
    n = 1 << log_n
    a = O.synth_scalars(fid, SEED | (0x100 + log_n), n).reshape(n, 4)
    w = limbs_arr(f, f.omega(log_n))
    want = O.best_fft(fid, a, w, log_n, threads=8).reshape(n, 4)
    d = dev(a)
    h2.ntt_device(d.data_ptr(), 1, w, log_n, curve)
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy().view(np.uint64), want)
    # EvaluationDomain::ifft: omega^-1 and the constant 1 / n (in the final pass, or in the inter-pass twiddles)
    wi = limbs_arr(f, pow(f.omega(log_n), -1, f.p))
    cm = limbs_arr(f, pow(n, -1, f.p))
    plain = O.best_fft(fid, a, wi, log_n, threads=8)
    want_inv = O.field_mul_many(fid, plain.reshape(-1), np.tile(cm, n)).reshape(n, 4)
    d = dev(a)
    assert L.h2_ntt_scaled_device(CID[curve], ctypes.c_void_p(d.data_ptr()), 1, wi.ctypes.data, log_n, cm.ctypes.data, None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy().view(np.uint64), want_inv)


def zeta_of(curve):
    from halo2_prover_amd.domain import _FIELDS
    p, gen, _, zeta = _FIELDS[CID[curve]]
    z = zeta if zeta is not None else pow(gen, (p - 1) // 3, p)
    assert z != 1 and pow(z, 3, p) == 1
    return z


@pytest.mark.parametrize("curve", PASTA_CURVES)
def test_coeff_to_extended_and_back_against_the_oracle(h2, curve):
    """(k, extended k) = (8, 11), two columns.  Forward: FFT of the zero-padded coefficients times zeta^i.  Back: the
    values times t[i mod 8], the inverse transform, 1 / 2^11 and zeta^-j, the first 3/4 kept"""
    import torch
    from halo2_prover_amd import lib
    f, fid, cid = scalar_field(curve), fid_of(curve), CID[curve]
    L = lib.load()
    k, e, m = 8, 11, 2
    n, en = 1 << k, 1 << e
    z = zeta_of(curve)
    zi = pow(z, -1, f.p)
    coeffs = np.stack([O.synth_scalars(fid, SEED | (0x200 + c), n).reshape(n, 4) for c in range(m)])
    zpow = np.stack([limbs_arr(f, pow(z, i % 3, f.p)) for i in range(n)])
    w = limbs_arr(f, f.omega(e))
    want_ext = []
    for c in range(m):
        padded = np.zeros((en, 4), dtype=np.uint64)
        padded[:n] = O.field_mul_many(fid, coeffs[c].reshape(-1), zpow.reshape(-1)).reshape(n, 4)
        want_ext.append(O.best_fft(fid, padded, w, e, threads=8).reshape(en, 4))
    want_ext = np.stack(want_ext)
    src = dev(coeffs)
    ext = torch.full((m, en, 4), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    zl = limbs_arr(f, z)
    lib.check(L.h2_coeff_to_extended_device(cid, ctypes.c_void_p(src.data_ptr()), n, k, m, zl.ctypes.data, w.ctypes.data, e,
                                            ctypes.c_void_p(ext.data_ptr()), None), "h2_coeff_to_extended_device")
    torch.cuda.synchronize()
    assert np.array_equal(ext.cpu().numpy().view(np.uint64), want_ext)

    period, out_len = 8, 3 * en // 4
    t = np.stack([O.synth_scalars(fid, SEED | 0x300, period).reshape(period, 4)])[0]
    wi = limbs_arr(f, pow(f.omega(e), -1, f.p))
    sc = limbs_arr(f, pow(en, -1, f.p))
    zil = limbs_arr(f, zi)
    tail = np.stack([limbs_arr(f, pow(en, -1, f.p) * pow(zi, j % 3, f.p) % f.p) for j in range(en)])
    want_back = []
    for c in range(m):
        x = O.field_mul_many(fid, want_ext[c].reshape(-1), np.tile(t, (en // period, 1)).reshape(-1))
        y = O.best_fft(fid, x, wi, e, threads=8)
        want_back.append(O.field_mul_many(fid, y.reshape(-1), tail.reshape(-1)).reshape(en, 4)[:out_len])
    want_back = np.stack(want_back)
    td = dev(t)
    out = torch.full((m, out_len, 4), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    lib.check(L.h2_extended_to_coeff_device(cid, ctypes.c_void_p(ext.data_ptr()), e, m, wi.ctypes.data, sc.ctypes.data,
                                            zil.ctypes.data, ctypes.c_void_p(td.data_ptr()), period,
                                            ctypes.c_void_p(out.data_ptr()), out_len, out_len, None),
              "h2_extended_to_coeff_device")
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint64), want_back)
