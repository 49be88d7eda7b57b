"""GPU: the MSM's sort front and launch glue at the smallest shapes that reach each path.

* staged scatter with packed 4-byte entries and tiles chosen per column: n = 2^12 / 2^13, m = 3, 5, 6, 7 (column counts
  that do not divide 256), a short last tile under a prefix of the bases, per-column bases;
* hot tasks summed inside the fix-up launch: a column whose scalars are all equal puts every window's 8192 entries
  into one bucket, cut into ~1000 pieces, beside a uniform and an all-zero column; repeated on the same workspace after
  a launch of another shape;
* the unpacked staged entry, forced through guard mode 3;
* the roofline profile of two launches (h2_profile_read).
Every launch runs in guard mode (a red zone behind every region of the arena, tests/test_gpu_msm_geometry.py) where the
test is about indices, and every result is compared with the CPU oracle.
"""
import ctypes
import time

import numpy as np
import pytest

import oracle_lib as O
import pyref as R

pytestmark = pytest.mark.gpu
SEED = 0x48324D5346000000
CID = O.CURVE_IDS
_BASES = {}


def scalars(curve, n, seed):
    return O.synth_scalars(O.CURVE_SCALAR_FIELD[CID[curve]], SEED | seed, n).reshape(n, 4)


def bases_of(curve, n, seed=0xB7):
    """host copy of the synthetic bases, computed once per (curve, n, seed) and never modified"""
    key = (curve, n, seed)
    if key not in _BASES:
        b = O.synth_bases(CID[curve], SEED | seed, n, threads=8).reshape(n, 8)
        b.setflags(write=False)
        _BASES[key] = b
    return _BASES[key]


def want(curve, col, b):
    return O.to_affine(CID[curve], O.best_multiexp(CID[curve], np.ascontiguousarray(col), np.ascontiguousarray(b), threads=8))


def guard_report(lib):
    out = (ctypes.c_uint64 * 2)()
    first = ctypes.create_string_buffer(256)
    assert lib.h2_selftest_msm_guard_report(out, first, 256) == 0
    return int(out[0]), int(out[1]), first.value.decode()


def front(lib, curve, n_bases, n, m, pack=1):
    """the sort front of the launch as the library lays it out (host side; tests/test_msm_front.py)"""
    out = (ctypes.c_uint64 * 12)()
    assert lib.h2_selftest_msm_front(CID[curve], n_bases, n, m, pack, out) == 0
    keys = ("tile", "staged", "stage_lds", "packed", "bbits", "ibits", "wbits", "ok", "T", "hot_span", "hot_seg", "max_tasks")
    return dict(zip(keys, [int(x) for x in out]))


@pytest.fixture()
def guarded(h2):
    lib = h2.load()
    lib.h2_selftest_msm_guard(1)
    yield lib
    lib.h2_selftest_msm_guard(0)


@pytest.mark.parametrize("m", [3, 5, 6, 7])
@pytest.mark.parametrize("log_n", [12, 13])
@pytest.mark.parametrize("curve", ["pallas", "bn254"])
def test_packed_staged_scatter(h2, guarded, curve, log_n, m):
    lib = guarded
    n = 1 << log_n
    f = front(lib, curve, n, n, m)
    assert f["staged"] == 1 and f["packed"] == 1                 # the path this test is about
    b = bases_of(curve, n)
    bases = h2.Bases(curve, b)
    try:
        cols = [scalars(curve, n, 0x100 * log_n + 16 * m + j) for j in range(m)]
        cols[1][n // 2:] = 0                                       # fewer entries than the worst case
        got = bases.msm_batch(cols)
        launches, violations, first = guard_report(lib)
        assert launches >= 1 and violations == 0, first
        for j in range(m):
            assert np.array_equal(got[j], want(curve, cols[j], b)), j
    finally:
        bases.release()


def test_unpacked_staged_scatter(h2):
    """the 4 + 2 byte staged entry, which no current geometry selects by itself: forced by guard mode 3"""
    lib = h2.load()
    curve, n, m = "pallas", 1 << 12, 5
    f = front(lib, curve, n, n, m, pack=0)
    assert f["staged"] == 1 and f["packed"] == 0
    b = bases_of(curve, n)
    bases = h2.Bases(curve, b)
    lib.h2_selftest_msm_guard(3)
    try:
        cols = [scalars(curve, n, 0x800 + j) for j in range(m)]
        got = bases.msm_batch(cols)
        launches, violations, first = guard_report(lib)
        assert launches >= 1 and violations == 0, first
        for j in range(m):
            assert np.array_equal(got[j], want(curve, cols[j], b)), j
    finally:
        lib.h2_selftest_msm_guard(0)
        bases.release()


def test_short_last_tile_under_a_prefix_of_the_bases(h2, guarded):
    lib = guarded
    curve, n_bases, m = "pallas", 1 << 13, 5
    n = n_bases - 1237
    f = front(lib, curve, n_bases, n, m)                           # the launch's own layout: n scalars, n_bases bases
    assert f["staged"] == 1 and f["packed"] == 1
    assert n % f["tile"] != 0                                      # the last tile of every column is short
    b = bases_of(curve, n_bases)
    bases = h2.Bases(curve, b)
    try:
        cols = [scalars(curve, n, 0x900 + j) for j in range(m)]
        got = bases.msm_batch(cols)
        launches, violations, first = guard_report(lib)
        assert launches >= 1 and violations == 0, first
        for j in range(m):
            assert np.array_equal(got[j], want(curve, cols[j], b[:n])), j
    finally:
        bases.release()


def test_per_column_bases_through_the_packed_scatter(h2, guarded):
    import torch
    from halo2_prover_amd import api
    lib = guarded
    curve, n, m = "bn254", 1 << 12, 3
    assert front(lib, curve, n, n, m)["packed"] == 1
    ba, bb = bases_of(curve, n), bases_of(curve, n, 0xB8)
    A, B = h2.Bases(curve, ba), h2.Bases(curve, bb)
    try:
        cols = np.stack([scalars(curve, n, 0xA00 + j) for j in range(m)])
        d = torch.from_numpy(cols.view(np.int64)).cuda()
        out = torch.zeros((m, 12), dtype=torch.int64, device="cuda")
        which = [A, B, A]
        api.msm_device_multi(which, d.data_ptr(), 0, n, n, out.data_ptr())
        torch.cuda.synchronize()
        launches, violations, first = guard_report(lib)
        assert launches >= 1 and violations == 0, first
        res = out.cpu().numpy().view(np.uint64)
        for j in range(m):
            assert np.array_equal(O.to_affine(CID[curve], res[j]), want(curve, cols[j], ba if which[j] is A else bb)), j
    finally:
        A.release()
        B.release()


def test_hot_buckets_are_summed_inside_the_fixup_launch(h2):
    """no guard mode here: its fill would hide what the test is about, the zeroed region handed from one launch
    sequence to the next on the same workspace"""
    curve, n, m = "pallas", 1 << 13, 3
    lay = front(h2.load(), curve, n, n, m)
    # a column of equal scalars puts the n entries of a non-zero window into one bucket: at least ceil(n / T) pieces
    # (T is largest when every digit is non-zero), which must be past the threshold of the hot-task path
    pieces = -(-n // lay["T"])
    assert pieces > lay["hot_span"], lay
    assert 0 < -(-pieces // lay["hot_seg"]) <= lay["max_tasks"]     # so the launch emits tasks, and they have slots
    f = R.CURVES[curve].scalar
    b = bases_of(curve, n)
    other = bases_of(curve, 1 << 12)
    bases, small = h2.Bases(curve, b), h2.Bases(curve, other)
    try:
        const = np.tile(np.array(f.limbs(0x1234567ABCDEF << 150 | 0x6F3A59C1), dtype=np.uint64), (n, 1))
        cols = [const, scalars(curve, n, 0xC01), np.zeros((n, 4), dtype=np.uint64)]
        expect = [want(curve, c, b) for c in cols]
        assert not np.any(expect[2])                               # the all-zero column commits to the identity
        got = bases.msm_batch(cols)
        for j in range(m):
            assert np.array_equal(got[j], expect[j]), j
        side = [scalars(curve, 1 << 12, 0xC10 + j) for j in range(5)]
        got_side = small.msm_batch(side)                           # another shape on the same workspace
        assert np.array_equal(got_side[4], want(curve, side[4], other))
        again = bases.msm_batch(cols)
        for j in range(m):
            assert np.array_equal(again[j], expect[j]), ("repeat", j)
    finally:
        bases.release()
        small.release()


def test_profile_of_two_launches(h2):
    from halo2_prover_amd.lib import Profile
    import torch
    lib = h2.load()
    curve, n, m = "pallas", 1 << 13, 3
    b = bases_of(curve, n)
    bases = h2.Bases(curve, b)
    try:
        cols = np.stack([scalars(curve, n, 0xD00 + j) for j in range(m)])
        d = torch.from_numpy(cols.view(np.int64)).cuda()
        out = torch.zeros((m, 12), dtype=torch.int64, device="cuda")
        bases.msm_device(d.data_ptr(), n, m, out.data_ptr())        # first call: allocations are not timed below
        torch.cuda.synchronize()
        lib.h2_profile_enable(1)
        t0 = time.perf_counter()
        bases.msm_device(d.data_ptr(), n, m, out.data_ptr())
        bases.msm_device(d.data_ptr(), n, m, out.data_ptr())
        torch.cuda.synchronize()
        wall_ms = (time.perf_counter() - t0) * 1e3
        prof = Profile()
        assert lib.h2_profile_read(ctypes.byref(prof)) == 0
        print("launches %d kernel_ms %.4f wall_ms %.4f" % (prof.launches, prof.kernel_ms, wall_ms))
        assert prof.launches == 2
        assert 0 < prof.kernel_ms < wall_ms
        assert lib.h2_profile_read(ctypes.byref(prof)) == 0        # read clears
        assert prof.launches == 0 and prof.kernel_ms == 0
        res = out.cpu().numpy().view(np.uint64)
        assert np.array_equal(O.to_affine(CID[curve], res[1]), want(curve, cols[1], b))
    finally:
        lib.h2_profile_enable(0)
        bases.release()
