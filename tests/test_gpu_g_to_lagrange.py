"""GPU: h2_g_to_lagrange* and h2_params_downsize (include/h2hip.h) on the GLV group FFT (csrc/h2_group_fft.hpp).

Sizes: the stage kernel has 256 threads a block in both forms -- 64 butterflies a block with four lanes per butterfly,
256 with one.  log n = 7 is one full block of the four-lane form, 8 two, 9 four; log n = 9 is one full block of the
one-lane form and 10 two.  h2_selftest_set_gfft_lanes forces either form at these sizes.
"""
import ctypes
import hashlib

import numpy as np
import pytest

import oracle_lib as O
import pyref as R
from test_capi_product import ARITH_INPUT, PARAMS_SHA256, Stream, c_prove, c_setup, c_verify, golden

pytestmark = pytest.mark.gpu

CURVES = ["bn254", "pallas", "vesta"]
CID = O.CURVE_IDS
SEED = 0x48324D5300000000
QUAD_SIZES, LANE_SIZES = [0, 1, 2, 3, 7, 8, 9], [1, 3, 9, 10]
UNSCALED = {4: 8, 1: 9}                    # the size at which each form also runs with scale = 1
CASES = [(4, s) for s in QUAD_SIZES] + [(1, s) for s in LANE_SIZES]


@pytest.fixture(scope="module")
def lib(h2):
    return h2.load()


def mont(f, v):
    return np.array(f.limbs(v % f.p), dtype=np.uint64)


def domain_constants(curve, log_n):
    f = R.CURVES[curve].scalar
    return mont(f, pow(f.omega(log_n), -1, f.p)), mont(f, pow(1 << log_n, -1, f.p))


def exceptional_bases(curve, log_n):
    """test_group_fft_matches_oracle's recipe: random points and, from n = 8, the identity, a repeated point and a point
    beside its negative"""
    n = 1 << log_n
    c = R.CURVES[curve]
    aff = O.synth_bases(CID[curve], SEED | (0xC0 + log_n), n).reshape(n, 8)
    if n >= 8:
        aff[2] = 0
        aff[5] = aff[4]
        neg = aff[6].copy()
        y = c.base.from_mont(O.limbs_to_int(neg[4:]))
        neg[4:] = np.array(c.base.limbs((-y) % c.base.p), dtype=np.uint64)
        aff[7] = neg
    return aff


def affine_to_jac(curve, aff):
    f = R.CURVES[curve].base
    jac = np.zeros((aff.shape[0], 12), dtype=np.uint64)
    jac[:, :8] = aff
    jac[aff.any(axis=1), 8:] = np.array(f.limbs(1), dtype=np.uint64)
    return jac


_REFERENCE = {}


def reference(curve, log_n):
    """(inputs, the oracle's unscaled transform as Jacobian points), computed once per (curve, size) and never written"""
    key = (curve, log_n)
    if key not in _REFERENCE:
        aff = exceptional_bases(curve, log_n)
        w_inv, _ = domain_constants(curve, log_n)
        fft = O.group_fft(CID[curve], affine_to_jac(curve, aff).reshape(-1), w_inv, log_n)
        aff.setflags(write=False)
        fft.setflags(write=False)
        _REFERENCE[key] = (aff, fft)
    return _REFERENCE[key]


def run_device(lib, curve, aff, log_n, w_inv, scale, in_place):
    import torch
    d_in = torch.from_numpy(np.ascontiguousarray(aff).view(np.int64).copy()).cuda()
    d_out = d_in if in_place else torch.zeros_like(d_in)
    st = lib.h2_g_to_lagrange_device(CID[curve], ctypes.c_void_p(d_in.data_ptr()), log_n, w_inv.ctypes.data, scale.ctypes.data,
                                     ctypes.c_void_p(d_out.data_ptr()), None)
    assert st == 0, (st, lib.h2_last_device_error())
    torch.cuda.synchronize()
    if not in_place:
        assert np.array_equal(d_in.cpu().numpy().view(np.uint64), aff)          # the input is read only
    return d_out.cpu().numpy().view(np.uint64).reshape(-1, 8)


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("lanes,log_n", CASES)
def test_matches_the_oracle_byte_for_byte(lib, curve, lanes, log_n):
    """O.group_fft with omega^-1, then O.scalar_mul by the scale, then O.to_affine -- against the affine output, once out
    of place and once in place, with both forms of the stage kernel"""
    n = 1 << log_n
    f = R.CURVES[curve].scalar
    aff, fft = reference(curve, log_n)
    w_inv, n_inv = domain_constants(curve, log_n)
    scales = [n_inv] + ([mont(f, 1)] if UNSCALED[lanes] == log_n else [])
    assert lib.h2_selftest_set_gfft_lanes(lanes) == 0
    try:
        for scale in scales:
            want = O.to_affine(CID[curve], O.scale_points(CID[curve], scale, fft)).reshape(n, 8)
            for in_place in (False, True):
                got = run_device(lib, curve, aff, log_n, w_inv, scale, in_place)
                assert np.array_equal(got, want), (in_place, scale.tolist())
    finally:
        lib.h2_selftest_set_gfft_lanes(0)


def test_oracle_scale_points_is_scalar_mul():
    """the expected values above scale with O.scale_points; it is O.scalar_mul point by point"""
    aff, _ = reference("bn254", 3)
    _, n_inv = domain_constants("bn254", 3)
    jac = affine_to_jac("bn254", aff)
    got = O.to_affine(0, O.scale_points(0, n_inv, jac.reshape(-1))).reshape(8, 8)
    for i in range(8):
        assert np.array_equal(got[i], O.to_affine(0, O.scalar_mul(0, n_inv, aff[i])))


# ------------------------------------------------------------------- the reference's own SRS ----
@pytest.fixture(scope="module")
def blob11(lib):
    blob = c_setup(lib, 11, Stream(0))
    assert hashlib.sha256(blob).hexdigest() == PARAMS_SHA256[11]
    return blob


def parts(blob):
    k = int.from_bytes(blob[:4], "little")
    n = 1 << k
    g = np.frombuffer(blob, dtype=np.uint64, count=8 * n, offset=4).reshape(n, 8).copy()
    gl = np.frombuffer(blob, dtype=np.uint64, count=8 * n, offset=4 + 64 * n).reshape(n, 8).copy()
    return k, g, gl


def downsize(lib, blob, k, expect=0):
    n = ctypes.c_size_t(0)
    cap = 4 + 128 * (1 << min(k, 26)) + 256
    out = ctypes.create_string_buffer(cap)
    rc = lib.h2_params_downsize(blob, len(blob), k, out, cap, ctypes.byref(n))
    assert rc == expect, (rc, lib.h2_last_device_error())
    return out.raw[:n.value]


def test_g_lagrange_of_the_recorded_srs(h2, lib, blob11):
    """h2_g_to_lagrange of the recorded blob's g is its g_lagrange, byte for byte: lanes by size at k = 11, both forms at
    k = 10 (the k = 10 blob is the k = 11 blob cut down: same stream, same s)"""
    _, g, gl = parts(blob11)
    assert np.array_equal(h2.g_to_lagrange(g, 11), gl)
    blob10 = downsize(lib, blob11, 10)
    assert hashlib.sha256(blob10).hexdigest() == PARAMS_SHA256[10]
    _, g10, gl10 = parts(blob10)
    assert np.array_equal(g10, g[:1024])
    try:
        for lanes in (1, 4):
            assert lib.h2_selftest_set_gfft_lanes(lanes) == 0
            assert np.array_equal(h2.g_to_lagrange(g10, 10), gl10), lanes
    finally:
        lib.h2_selftest_set_gfft_lanes(0)


@pytest.mark.parametrize("k", [10, 6, 4])
def test_downsize_reproduces_the_recorded_params(h2, lib, blob11, k):
    small = downsize(lib, blob11, k)
    assert hashlib.sha256(small).hexdigest() == PARAMS_SHA256[k]
    if k in (4, 6):
        assert small == golden("params_k%d.bin" % k)
    assert h2.params_downsize(blob11, k) == small


def test_downsize_to_the_blobs_own_k_recomputes_g_lagrange(h2, lib):
    p6 = golden("params_k6.bin")
    assert downsize(lib, p6, 6) == p6
    params = h2.ParamsKZG.read(p6).downsize(4)
    assert params.write() == golden("params_k4.bin")


def test_the_arithmetic_proof_under_a_downsized_blob(h2, lib, blob11):
    p4 = downsize(lib, downsize(lib, blob11, 10), 4)
    proof = c_prove(lib, p4, ARITH_INPUT, 1, Stream(8))
    assert proof == golden("proof_arithmetic_k4.bin")
    assert c_verify(lib, p4, proof, ARITH_INPUT, 1) == (0, 1)


# ------------------------------------------------------ Pasta at a multi-block size, no oracle FFT ----
def test_pallas_lagrange_basis_identities(h2, lib):
    """out = g_lagrange of 1024 random Pallas points: sum_i out[i] = g[0], sum_i omega^i out[i] = g[1], and
    commit_lagrange(col) over out = commit(ifft(col)) over g -- sums by h2_msm_points"""
    curve, log_n = "pallas", 10
    n = 1 << log_n
    f = R.CURVES[curve].scalar
    fid = O.CURVE_SCALAR_FIELD[CID[curve]]
    g = O.synth_bases(CID[curve], SEED | 0xD7, n).reshape(n, 8)
    out = h2.g_to_lagrange(g, log_n, curve)

    def norm(jac):
        return O.to_affine(CID[curve], jac)
    ones = np.tile(mont(f, 1), (n, 1))
    assert np.array_equal(norm(h2.msm_points(ones, out, curve)), g[0])
    w = f.omega(log_n)
    powers = np.stack([mont(f, pow(w, i, f.p)) for i in range(n)])
    assert np.array_equal(norm(h2.msm_points(powers, out, curve)), g[1])
    col = O.synth_scalars(fid, SEED | 0xD8, n).reshape(n, 4)
    w_inv, n_inv = domain_constants(curve, log_n)
    coeff = col.copy()
    h2.best_fft(coeff, w_inv, log_n, curve)
    coeff = O.field_mul_many(fid, coeff.reshape(-1), np.tile(n_inv, n)).reshape(n, 4)
    assert np.array_equal(norm(h2.msm_points(col, out, curve)), norm(h2.msm_points(coeff, g, curve)))


# ------------------------------------------------------------------------------------ errors ----
def test_bad_arguments_are_status_codes(h2, lib, blob11):
    import torch
    w_inv, n_inv = domain_constants("bn254", 4)
    d = torch.zeros(2 * 16 * 8 + 8, dtype=torch.int64, device="cuda")
    p = d.data_ptr()
    assert p % 16 == 0
    W, S = w_inv.ctypes.data, n_inv.ctypes.data

    def call(curve=0, d_in=p, log_n=4, w=W, s=S, d_out=p):
        return lib.h2_g_to_lagrange_device(curve, ctypes.c_void_p(d_in) if d_in else None, log_n, w, s,
                                           ctypes.c_void_p(d_out) if d_out else None, None)
    assert call() == 0                                         # the identity everywhere: a valid call
    assert call(curve=7) == -1
    assert call(d_in=0) == -1
    assert call(d_out=0) == -1
    assert call(w=None) == -1
    assert call(s=None) == -1
    assert call(d_in=p + 8, d_out=p + 8) == -1                 # not 16-byte aligned
    assert call(d_out=p + 16 * 64 + 8) == -1
    assert call(log_n=27) == -1
    assert call(d_out=p + 64) == -1                            # a partial overlap
    assert call(d_out=p + 16 * 64) == 0                        # the ranges touch, they do not overlap
    torch.cuda.synchronize()
    g = np.zeros((16, 8), dtype=np.uint64)
    assert lib.h2_g_to_lagrange(0, None, 4, W, S, g.ctypes.data) == -1
    assert lib.h2_g_to_lagrange(0, g.ctypes.data, 27, W, S, g.ctypes.data) == -1
    p6 = golden("params_k6.bin")
    downsize(lib, p6, 7, expect=-1)                            # k above the blob's
    downsize(lib, p6, 0, expect=-1)
    n = ctypes.c_size_t(0)
    out = ctypes.create_string_buffer(len(p6))
    assert lib.h2_params_downsize(p6[:-1], len(p6) - 1, 4, out, len(p6), ctypes.byref(n)) == -6      # one byte short
    assert lib.h2_params_downsize(p6, 3, 4, out, len(p6), ctypes.byref(n)) == -6
    assert lib.h2_params_downsize(p6, len(p6), 4, out, 16, ctypes.byref(n)) == -1                    # no room:
    assert n.value == 4 + 128 * 16 + 256                                                             # how much is needed
    with pytest.raises(ValueError):
        h2.g_to_lagrange(g, 5)
    with pytest.raises(ValueError):
        h2.ParamsKZG.read(golden("params_k4.bin")).downsize(5)
