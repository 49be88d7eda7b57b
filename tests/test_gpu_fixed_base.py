"""GPU: the two fixed-base setup kernels, h2_fixed_base_mul ([k_i] G) and h2_srs_generate ([s^i] G), on BN254, Pallas and
Vesta.  The double-and-add of both walks a scalar's bits from 255 down on the curve's generator (CV::GX / CV::GY) and
leaves through xyzz_to_affine; the expected points come from the big-integer group law (pyref) for scalars chosen by
their bit patterns, and from the CPU oracle (pinned through its field arithmetic and, here, against pyref) for random
ones.  Outputs are affine Montgomery limbs, unique per point: every comparison is bytewise; the identity is 64 zero
bytes.
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


def scalar_limbs(f, vals):
    return np.array([f.limbs(v) for v in vals], dtype=np.uint64).reshape(len(vals), 4)


def affine(c, pts):
    return np.frombuffer(b"".join(c.affine_bytes(P) for P in pts), dtype=np.uint64).reshape(len(pts), 8).copy()


def guarded_out(n):
    """n affine points (8 limbs each) of sentinel fill and GUARD more behind them"""
    import torch
    full = np.full((n + GUARD, 8), SENTINEL, dtype=np.uint64)
    return torch.from_numpy(full.view(np.int64)).cuda()


def fetch(buf, n):
    import torch
    torch.cuda.synchronize()
    h = buf.cpu().numpy().view(np.uint64)
    assert (h[n:] == SENTINEL).all(), "guard behind the output was written"
    return h[:n]


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def fixed_base_mul(h2, curve, k_limbs, stream=None):
    import torch
    n = k_limbs.shape[0]
    d_k = torch.from_numpy(k_limbs.view(np.int64)).cuda()
    out = guarded_out(n)
    assert h2.load().h2_fixed_base_mul(CID[curve], ptr(d_k), n, ptr(out), stream) == 0
    got = fetch(out, n)
    assert np.array_equal(d_k.cpu().numpy().view(np.uint64), k_limbs)          # the scalars are read only
    return got


def srs_generate(h2, curve, s, n):
    f = R.CURVES[curve].scalar
    out = guarded_out(n)
    s_m = scalar_limbs(f, [s])
    assert h2.load().h2_srs_generate(CID[curve], s_m.ctypes.data, n, ptr(out), None) == 0
    return fetch(out, n)


def oracle_fixed_base(curve, k_limbs):
    c = R.CURVES[curve]
    g = affine(c, [c.gen]).reshape(8)
    return np.stack([O.to_affine(CID[curve], O.scalar_mul(CID[curve], k, g)) for k in k_limbs])


@pytest.mark.parametrize("curve", CURVES)
def test_fixed_base_mul_bit_patterns(h2, curve):
    """scalars that walk the branches of the double-and-add: 0 (the identity, (0, 0) out of xyzz_to_affine), 1 (one
    addition into the identity), 2 and 3, r - 1 = -1 and r - 2, the two halves, single bits at the 32- and 64-bit limb
    borders and at the top, 2^255 mod r, the alternating patterns, then random scalars; against pyref's group law"""
    c = R.CURVES[curve]
    r = c.scalar.p
    rng = random.Random(100 + CID[curve])
    ks = [0, 1, 2, 3, r - 1, r - 2, (r - 1) // 2, (r + 1) // 2] + [1 << k for k in (31, 32, 63, 64, 128, 253)]
    ks += [(1 << 255) % r, int("AA" * 32, 16) % r, int("55" * 32, 16) % r]
    ks += [rng.randrange(r) for _ in range(36 - len(ks))]
    want = affine(c, [c.mul(k, c.gen) for k in ks])
    assert not want[0].any() and np.array_equal(want[1], affine(c, [c.gen])[0])
    assert np.array_equal(want[4], affine(c, [c.neg(c.gen)])[0])
    got = fixed_base_mul(h2, curve, scalar_limbs(c.scalar, ks))
    assert np.array_equal(got, want)
    assert O.is_on_curve(CID[curve], got)


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_fixed_base_mul_block_boundary(h2, curve, n):
    """one thread per scalar, 256 per block: n around the block, random scalars (with 0 and r - 1 among them: the
    oracle's to_affine gives 64 zero bytes for the identity, as pyref does), a guard behind the output"""
    c = R.CURVES[curve]
    k = O.synth_scalars(O.CURVE_SCALAR_FIELD[CID[curve]], 0x48324D5300006000 + n, n).reshape(n, 4).copy()
    if n > 1:
        k[n // 2] = 0
        k[n - 1] = scalar_limbs(c.scalar, [c.scalar.p - 1])[0]
    want = oracle_fixed_base(curve, k)
    if n > 1:
        assert not want[n // 2].any() and np.array_equal(want[n - 1], affine(c, [c.neg(c.gen)])[0])
    assert np.array_equal(fixed_base_mul(h2, curve, k), want)


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("n", [1, 2, 257])
def test_srs_generate(h2, curve, n):
    """g[i] = [s^i] G against the oracle's powers_of_s (checked against pyref on the first 16 rows here), and the closed
    forms: s = 0 gives G then the identity (fe_pow_u64(0, 0) = 1), s = 1 gives G everywhere, s = r - 1 alternates G and -G"""
    c = R.CURVES[curve]
    r, cid = c.scalar.p, CID[curve]
    G, negG, ident = affine(c, [c.gen])[0], affine(c, [c.neg(c.gen)])[0], np.zeros(8, dtype=np.uint64)
    for s in (0, 1, r - 1, 2, 0x1234567890ABCDEF1122334455667788AABBCCDD % r):
        want = O.to_affine(cid, O.powers_of_s(cid, scalar_limbs(c.scalar, [s]), n)).reshape(n, 8)
        head = min(n, 16)
        assert np.array_equal(want[:head], affine(c, [c.mul(pow(s, i, r), c.gen) for i in range(head)]))
        got = srs_generate(h2, curve, s, n)
        assert np.array_equal(got, want), hex(s)
        if s == 0:
            assert np.array_equal(got[0], G) and not got[1:].any()
        elif s == 1:
            assert np.array_equal(got, np.tile(G, (n, 1)))
        elif s == r - 1:
            assert np.array_equal(got, np.stack([G if i % 2 == 0 else negG for i in range(n)]))
        else:
            assert not (got == ident).all(axis=1).any()


@pytest.mark.parametrize("curve", CURVES)
def test_the_two_kernels_agree(h2, curve):
    """h2_fixed_base_mul on the column s^i is h2_srs_generate(s), byte for byte"""
    f = R.CURVES[curve].scalar
    n = 257
    for s in (f.p - 1, 0xFEDCBA9876543210FEDCBA9876543210FEDCBA98 % f.p):
        col, cur = [], 1
        for _ in range(n):
            col.append(cur)
            cur = cur * s % f.p
        assert np.array_equal(fixed_base_mul(h2, curve, scalar_limbs(f, col)), srs_generate(h2, curve, s, n)), hex(s)


def test_fixed_base_on_a_non_default_stream(h2):
    import torch
    curve, n = "vesta", 257
    k = O.synth_scalars(O.CURVE_SCALAR_FIELD[CID[curve]], 0x48324D5300006100, n).reshape(n, 4)
    want = fixed_base_mul(h2, curve, k)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        got = fixed_base_mul(h2, curve, k, ctypes.c_void_p(side.cuda_stream))
    assert np.array_equal(got, want)


def test_status_codes(h2):
    """n = 0, a null pointer and a curve id out of range are H2_EINVAL, rejected on the host: nothing is written"""
    import torch
    L = h2.load()
    f = R.BN_FR
    s = scalar_limbs(f, [5])
    d_k = torch.from_numpy(scalar_limbs(f, [1, 2, 3, 4]).view(np.int64)).cuda()
    out = guarded_out(4)
    bad = []
    for cid in (0, 1, 2):
        bad += [L.h2_srs_generate(cid, s.ctypes.data, 0, ptr(out), None), L.h2_srs_generate(cid, None, 4, ptr(out), None),
                L.h2_srs_generate(cid, s.ctypes.data, 4, None, None), L.h2_fixed_base_mul(cid, ptr(d_k), 0, ptr(out), None),
                L.h2_fixed_base_mul(cid, None, 4, ptr(out), None), L.h2_fixed_base_mul(cid, ptr(d_k), 4, None, None)]
    for cid in (3, 7, -1):
        bad += [L.h2_srs_generate(cid, s.ctypes.data, 4, ptr(out), None), L.h2_fixed_base_mul(cid, ptr(d_k), 4, ptr(out), None)]
    assert bad == [EINVAL] * len(bad)
    assert (fetch(out, 4) == SENTINEL).all()
    # still healthy after the refusals
    assert L.h2_fixed_base_mul(0, ptr(d_k), 4, ptr(out), None) == 0
    c = R.BN254
    assert np.array_equal(fetch(out, 4), affine(c, [c.mul(k, c.gen) for k in (1, 2, 3, 4)]))
