"""CPU: the sort front of the MSM, checked on the host for every proof-sized shape (no GPU).

The staged scatter runs one block per CU, so its launch should be a whole number of rounds of 256 blocks: the tiles per
column are chosen first and the tile from them.  A staged entry is one packed word (window, index in the tile, sign,
bucket) where those fields fit 32 bits, else a reference and a 16-bit bucket.  For n = 2^10 .. 2^17 and m = 1 .. 16,
whenever the staged scatter is chosen: the block count, the LDS, the packed fields and the bounds proof.
The device side of the same paths is tests/test_gpu_msm_front.py.
"""
import ctypes

import pytest

import halo2_prover_amd as h2

CU_LDS = 160 * 1024          # bytes of LDS a workgroup can get on one CU
CURVES = {"bn254": 0, "pallas": 1, "vesta": 2}


@pytest.fixture(scope="module")
def lib():
    return h2.load()


def front(lib, curve, n, m, pack=1):
    out = (ctypes.c_uint64 * 12)()
    assert lib.h2_selftest_msm_front(curve, n, n, m, pack, out) == 0, (curve, n, m)
    d = dict(zip(("tile", "staged", "stage_lds", "packed", "bbits", "ibits", "wbits", "ok"), [int(x) for x in out[:8]]))
    geo = (ctypes.c_uint64 * 8)()
    assert lib.h2_selftest_msm_check(curve, n, n, m, n, 0, geo) == 0, (curve, n, m, lib.h2_last_device_error())
    d["W"], d["B"] = int(geo[1]), int(geo[2])
    if pack:
        assert (int(geo[3]), int(geo[4])) == (d["tile"], d["staged"])
    return d


def blocks(n, m, tile):
    return -(-n // tile) * m


@pytest.mark.parametrize("curve", sorted(CURVES))
def test_every_staged_launch_is_whole_rounds_with_entries_that_fit(lib, curve):
    staged = packed = 0
    for k in range(10, 18):
        n = 1 << k
        for m in range(1, 17):
            f = front(lib, CURVES[curve], n, m)
            assert f["ok"] == 1, (n, m, lib.h2_last_device_error())       # msm_check returned null
            if not f["staged"]:
                continue
            staged += 1
            tile, W, B = f["tile"], f["W"], f["B"]
            assert 1 <= tile <= n
            assert blocks(n, m, tile) <= 2 * 256, (n, m, tile)            # two rounds of one block per CU at most
            assert f["stage_lds"] <= CU_LDS, (n, m, f)
            if f["packed"]:
                packed += 1
                # window | index in tile | bucket below the sign bit, every field wide enough for its largest value
                assert W <= 1 << f["wbits"] and tile <= 1 << f["ibits"] and B <= 1 << f["bbits"], (n, m, f)
                assert f["wbits"] + f["ibits"] + f["bbits"] + 1 <= 32, (n, m, f)
                assert f["stage_lds"] >= 8 * B + 4 * tile * W, (n, m, f)
            else:
                assert B <= 1 << 16                                       # the 6-byte form: reference + 16-bit bucket
                assert f["stage_lds"] >= 8 * B + 6 * tile * W, (n, m, f)
    assert staged > 20 and packed > 20


@pytest.mark.parametrize("curve", sorted(CURVES))
def test_the_unpacked_entry_is_laid_out_where_it_is_forced(lib, curve):
    """No geometry the staged scatter accepts today overflows the packed word (test above: packed == staged), so the
    6-byte form is reached through the test hook only: the same bounds must hold for it."""
    staged = 0
    for k in range(10, 18):
        n = 1 << k
        for m in range(1, 17):
            f = front(lib, CURVES[curve], n, m, pack=0)
            assert f["ok"] == 1, (n, m, lib.h2_last_device_error())
            assert f["packed"] == 0
            if not f["staged"]:
                continue
            staged += 1
            assert blocks(n, m, f["tile"]) <= 2 * 256, (n, m, f)
            assert 8 * f["B"] + 6 * f["tile"] * f["W"] <= f["stage_lds"] <= CU_LDS, (n, m, f)
            assert f["B"] <= 1 << 16
    assert staged > 20


def test_proof_shapes_at_2e16_take_one_round(lib):
    n = 1 << 16
    got = {}
    for m in (3, 4, 5, 6):
        f = front(lib, CURVES["pallas"], n, m)
        assert f["staged"] == 1 and f["packed"] == 1, (m, f)
        got[m] = blocks(n, m, f["tile"])
    assert got[3] == 255
    assert got[4] == 256
    assert got[5] <= 256 and got[6] <= 256
