"""CPU (no GPU): the GLV split the group FFT's twiddle kernel runs (csrc/h2_group_fft.hpp glv_split, constants from
tools/glv_constants.py), through its host instantiation, against Python integers -- and the ABI of the three entry
points that go with it (h2_g_to_lagrange_device, h2_g_to_lagrange, h2_params_downsize).

k = k1 + k2 lambda (mod r) must hold exactly for every scalar, and both magnitudes must stay below 2^GLV_BITS, the length
of the kernels' joint double-and-add: a magnitude beyond it would lose its top bits there."""
import ctypes
import os
import random
import re

import numpy as np
import pytest

import pyref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CURVES = {"bn254": 0, "pallas": 1, "vesta": 2}
ENTRY_POINTS = {"h2_g_to_lagrange_device": 7, "h2_g_to_lagrange": 6, "h2_params_downsize": 6}


@pytest.fixture(scope="module")
def lib():
    import halo2_prover_amd
    return halo2_prover_amd.load()


def limbs(v):
    return (ctypes.c_uint64 * 4)(*[(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)])


def constants(lib, curve):
    """(lambda, beta, GLV_BITS) as the library reports them; beta out of its Montgomery form"""
    lam, beta, bits = (ctypes.c_uint64 * 4)(), (ctypes.c_uint64 * 4)(), ctypes.c_uint32(0)
    assert lib.h2_selftest_glv_constants(CURVES[curve], lam, beta, ctypes.byref(bits)) == 0
    f = R.CURVES[curve].base
    return sum(int(x) << (64 * i) for i, x in enumerate(lam)), f.from_mont(sum(int(x) << (64 * i) for i, x in enumerate(beta))), bits.value


def split(lib, curve, k):
    """(k1, k2) as signed integers and the larger bit length of the two magnitudes"""
    out = (ctypes.c_uint32 * 10)()
    assert lib.h2_selftest_glv_split(CURVES[curve], limbs(k), out) == 0
    vals = []
    for words in (out[:5], out[5:]):
        neg = words[4] >> 31
        mag = sum((w & (0x7FFFFFFF if i == 4 else 0xFFFFFFFF)) << (32 * i) for i, w in enumerate(words))
        vals.append((-mag if neg else mag, mag.bit_length()))
    return vals[0][0], vals[1][0], max(vals[0][1], vals[1][1])


@pytest.mark.parametrize("curve", sorted(CURVES))
def test_cube_roots_of_unity(lib, curve):
    c = R.CURVES[curve]
    lam, beta, bits = constants(lib, curve)
    assert 1 < lam < c.scalar.p and (lam * lam + lam + 1) % c.scalar.p == 0
    assert 1 < beta < c.base.p and (beta * beta + beta + 1) % c.base.p == 0
    assert 127 <= bits <= 159          # half the scalar's length, within the five words a magnitude is stored in


@pytest.mark.parametrize("curve", sorted(CURVES))
def test_beta_pairs_with_lambda_on_the_generator(lib, curve):
    """(beta x, y) = [lambda](x, y): the other cube root of either field would give [lambda^2]"""
    c = R.CURVES[curve]
    lam, beta, _ = constants(lib, curve)
    gx, gy = c.gen
    assert c.mul(lam, c.gen) == (beta * gx % c.base.p, gy)


@pytest.mark.parametrize("curve", sorted(CURVES))
def test_split_is_exact_and_short(lib, curve):
    f = R.CURVES[curve].scalar
    r = f.p
    lam, _, bits = constants(lib, curve)
    w = f.omega(10)
    scalars = [0, 1, 2, r - 1, lam, lam * lam % r, r - lam]
    scalars += [pow(w, i, r) for i in range(512)]                  # the twiddles of the 2^10 domain
    rng = random.Random(0x474C5600 + CURVES[curve])
    scalars += [rng.randrange(r) for _ in range(2000)]
    longest = 0
    for k in scalars:
        k1, k2, length = split(lib, curve, k)
        assert (k1 + k2 * lam - k) % r == 0, hex(k)
        assert length <= bits, (hex(k), length)
        longest = max(longest, length)
    assert longest >= 120              # and it IS a split: neither half is the scalar itself


def test_generated_constants_are_the_committed_ones():
    """tools/glv_constants.py derives what csrc/h2_glv_constants.inc holds (pairing check against the oracle included)"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("glv_constants", os.path.join(ROOT, "tools", "glv_constants.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    committed = open(os.path.join(ROOT, "halo2_prover_amd", "csrc", "h2_glv_constants.inc")).read()
    assert mod.cpp_inc() == committed


@pytest.mark.parametrize("name", sorted(ENTRY_POINTS))
def test_entry_points_are_exported_listed_and_declared(lib, name):
    import halo2_prover_amd
    assert hasattr(lib, name)
    res, args = halo2_prover_amd.SYMBOLS[name]
    assert res is ctypes.c_int and len(args) == ENTRY_POINTS[name]
    text = open(os.path.join(ROOT, "include", "h2hip.h")).read()
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, "include/h2hip.h does not declare " + name
    assert len(re.sub(r"/\*.*?\*/", "", m.group(1)).split(",")) == ENTRY_POINTS[name]
    assert lib.h2_version() == 1002


def test_loader_signatures():
    import halo2_prover_amd
    I, P, Z, U = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32
    S = halo2_prover_amd.SYMBOLS
    assert S["h2_g_to_lagrange_device"] == (I, [I, P, U, P, P, P, P])
    assert S["h2_g_to_lagrange"] == (I, [I, P, U, P, P, P])
    assert S["h2_params_downsize"][1][:5] == [P, Z, U, P, Z]
    assert S["h2_selftest_set_gfft_lanes"] == (I, [I])
    for name in ("g_to_lagrange", "params_downsize"):
        assert callable(getattr(halo2_prover_amd, name))
    assert callable(halo2_prover_amd.ParamsKZG.downsize)


def test_they_fail_loudly_without_init(lib):
    """no CPU fallback: before h2_init the calls are H2_ENOTINIT (with the null pointers passed here H2_EINVAL, and
    H2_EPROOF for the null blob, if another test of this process has initialised a device)"""
    z = (ctypes.c_uint64 * 4)(1, 0, 0, 0)
    n = ctypes.c_size_t(0)
    assert lib.h2_g_to_lagrange_device(0, None, 4, z, z, None, None) in (-5, -1)
    assert lib.h2_g_to_lagrange(0, None, 4, z, z, None) in (-5, -1)
    assert lib.h2_params_downsize(None, 0, 4, None, 0, ctypes.byref(n)) in (-5, -6)
    import torch
    if not torch.cuda.is_available():
        blob = open(os.path.join(ROOT, "tests", "golden", "params_k4.bin"), "rb").read()
        out = ctypes.create_string_buffer(len(blob))
        g = np.frombuffer(blob, dtype=np.uint64, count=8 * 16, offset=4).copy()
        assert lib.h2_g_to_lagrange(0, g.ctypes.data, 4, z, z, g.ctypes.data) == -5
        assert lib.h2_params_downsize(blob, len(blob), 4, out, len(blob), ctypes.byref(n)) == -5


def test_lane_knob_takes_only_its_three_values(lib):
    try:
        assert lib.h2_selftest_set_gfft_lanes(1) == 0
        assert lib.h2_selftest_set_gfft_lanes(4) == 0
        assert lib.h2_selftest_set_gfft_lanes(2) == -1
        assert lib.h2_selftest_set_gfft_lanes(-1) == -1
    finally:
        assert lib.h2_selftest_set_gfft_lanes(0) == 0
