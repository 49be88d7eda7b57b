"""CPU: the host rule for the lanes per key of the MSM's fix-up kernel (msm_workspace), for every proof-sized shape.

msm_fixup_kernel gives each key F = 2^log_f lanes: every lane folds its share of the key's pieces by itself, then the
key's F / 4 quads add the lanes' partial sums.  The first stage is fastest at one wave per SIMD, so F is the largest power
of two with keys * F <= 65 536 lanes (1024 SIMDs of 64), never more lanes than a key is assumed to have pieces, and a
quad at least.  For n = 2^10 .. 2^20 and m = 1 .. 16 on the three curves: those bounds, through h2_selftest_msm_fixup.
The device side is tests/test_gpu_msm_fixup.py.
"""
import ctypes

import pytest

import halo2_prover_amd as h2

CURVES = {"bn254": 0, "pallas": 1, "vesta": 2}
ONE_WAVE_PER_SIMD = 1024 * 64


@pytest.fixture(scope="module")
def lib():
    return h2.load()


def fixup(lib, curve, n, m):
    out = (ctypes.c_uint64 * 4)()
    assert lib.h2_selftest_msm_fixup(curve, n, n, m, out) == 0, (curve, n, m, lib.h2_last_device_error())
    return dict(zip(("log_f", "lanes", "pieces", "T"), [int(x) for x in out]))


def pow2_at_least(x):
    return 1 << max(0, x - 1).bit_length()


@pytest.mark.parametrize("curve", sorted(CURVES))
def test_lanes_per_key_of_every_proof_sized_launch(lib, curve):
    seen = set()
    for k in range(10, 21):
        n = 1 << k
        for m in range(1, 17):
            f = fixup(lib, CURVES[curve], n, m)
            geo = (ctypes.c_uint64 * 8)()
            assert lib.h2_selftest_msm_check(CURVES[curve], n, n, m, n, 0, geo) == 0, (n, m, lib.h2_last_device_error())
            B = int(geo[2])
            F = 1 << f["log_f"]
            seen.add(F)
            assert 4 <= F <= 64, (n, m, f)                                   # whole quads inside one wave
            keys = f["lanes"] // F                                           # of the first launch, if the columns take several
            assert f["lanes"] == keys * F and keys % B == 0 and B <= keys <= m * B, (n, m, f)
            assert f["lanes"] <= ONE_WAVE_PER_SIMD or F == 4, (n, m, f)
            assert f["pieces"] >= 1 and f["T"] >= 8, (n, m, f)
            assert F <= max(4, pow2_at_least(f["pieces"])), (n, m, f)        # no more lanes than pieces, a quad at least
            # the LARGEST such F: the next one breaks one of the bounds
            assert F == 64 or 2 * F > pow2_at_least(f["pieces"]) or keys * 2 * F > ONE_WAVE_PER_SIMD, (n, m, f)
    assert len(seen) > 1, seen                                              # the rule is not a constant


def test_the_benchmark_step_launches(lib):
    """Poseidon k = 16 on Pallas: 2048 buckets a column; four columns land on exactly one wave per SIMD"""
    n = 1 << 16
    want = {3: 8, 4: 8, 5: 4}
    for m, F in want.items():
        f = fixup(lib, CURVES["pallas"], n, m)
        assert 1 << f["log_f"] == F, (m, f)
        assert f["lanes"] == m * 2048 * F
    assert fixup(lib, CURVES["pallas"], n, 4)["lanes"] == ONE_WAVE_PER_SIMD


def test_rejects_what_msm_front_rejects(lib):
    out = (ctypes.c_uint64 * 4)()
    assert lib.h2_selftest_msm_fixup(CURVES["pallas"], 1 << 12, 0, 3, out) != 0
    assert lib.h2_selftest_msm_fixup(CURVES["pallas"], 1 << 12, 1 << 13, 3, out) != 0
    assert lib.h2_selftest_msm_fixup(7, 1 << 12, 1 << 12, 3, out) != 0
