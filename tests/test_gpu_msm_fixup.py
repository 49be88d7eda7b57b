"""GPU: the two stages of the MSM's fix-up kernel at the smallest shapes that reach each of their paths.

msm_fixup_kernel gives a key F lanes (the host rule: tests/test_msm_fixup.py).  Stage 1: every lane folds pieces
lane, lane + F, ... of the key's bucket with the one-lane addition; stage 2: the key's F / 4 quads add their lanes'
partial sums in the quad form and a shuffle tree joins the quads.  At n = 2^12 / 2^13 a thread of the accumulate kernel
takes 8 - 10 sorted entries, so a bucket has tens of pieces and F is 16 - 64:

* uniform columns, one of them half zero (the device then cuts finer than the host assumed), m = 3 and 5;
* short lists: keys with 0 - 3 pieces -- the single-chunk path, lanes without a piece, piece counts no multiple of F;
* bases that are all one point, and P, -P alternating: the pieces of a bucket are small multiples of P, equal ones,
  inverse ones and the identity among them, so the doubling and cancelling branches of both additions run (at m = 16
  a lane has several pieces and they run in stage 1, at m = 3 one piece at most and they run in stage 2);
* another shape on the same workspace in between.
Launches run in guard mode (a red zone behind every region of the arena) where the test is about indices, and every
result is compared with the CPU oracle.  Hot buckets: tests/test_gpu_msm_front.py.
"""
import ctypes

import numpy as np
import pytest

import oracle_lib as O
import pyref as R

pytestmark = pytest.mark.gpu
SEED = 0x48324D5346580000
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


def layout(lib, curve, n, m):
    """the fix-up's share of the launch as the library lays it out, and the launch's windows (host side)"""
    out = (ctypes.c_uint64 * 4)()
    assert lib.h2_selftest_msm_fixup(CID[curve], n, n, m, out) == 0
    geo = (ctypes.c_uint64 * 8)()
    assert lib.h2_selftest_msm_check(CID[curve], n, n, m, n, 0, geo) == 0
    front = (ctypes.c_uint64 * 12)()
    assert lib.h2_selftest_msm_front(CID[curve], n, n, m, 1, front) == 0
    return {"F": 1 << int(out[0]), "lanes": int(out[1]), "pieces": int(out[2]), "T": int(out[3]),
            "c": int(geo[0]), "W": int(geo[1]), "B": int(geo[2]), "hot_span": int(front[9])}


def longest_bucket_list(col, c, W):
    """entries of the fullest bucket of a column under the textbook signed-digit recoding with c-bit windows (the
    library's own recoding may round a boundary digit the other way: a handful of entries either way)"""
    vals = [int(r[0]) | int(r[1]) << 64 | int(r[2]) << 128 | int(r[3]) << 192 for r in col]
    counts = np.zeros((1 << (c - 1)) + 1, dtype=np.int64)
    half, mask = 1 << (c - 1), (1 << c) - 1
    for v in vals:
        carry = 0
        for w in range(W + 1):
            d = ((v >> (c * w)) & mask) + carry
            carry = 1 if d > half else 0
            if carry:
                d -= 1 << c
            if d:
                counts[abs(d)] += 1
    return int(counts.max())


def one_point_bases(curve, n, alternate):
    """n copies of one point P; `alternate`: P, -P, P, ... (y -> p - y, in whatever form the limbs hold y)"""
    p = R.CURVES[curve].base.p
    P = bases_of(curve, 1 << 12)[5]
    b = np.tile(P, (n, 1))
    if alternate:
        y = sum(int(P[4 + i]) << (64 * i) for i in range(4))
        neg = p - y
        b[1::2, 4:] = np.array([(neg >> (64 * i)) & (2**64 - 1) for i in range(4)], dtype=np.uint64)
    return b


@pytest.fixture()
def guarded(h2):
    lib = h2.load()
    lib.h2_selftest_msm_guard(1)
    yield lib
    lib.h2_selftest_msm_guard(0)


def run_guarded(h2, lib, curve, b, cols):
    bases = h2.Bases(curve, b)
    try:
        got = bases.msm_batch(cols)
        launches, violations, first = guard_report(lib)
        assert launches >= 1 and violations == 0, first
        for j, col in enumerate(cols):
            assert np.array_equal(got[j], want(curve, col, b)), j
    finally:
        bases.release()


@pytest.mark.parametrize("m", [3, 5])
@pytest.mark.parametrize("log_n", [12, 13])
@pytest.mark.parametrize("curve", ["pallas", "bn254"])
def test_uniform_columns(h2, guarded, curve, log_n, m):
    n = 1 << log_n
    lay = layout(guarded, curve, n, m)
    assert lay["T"] <= 10 and lay["pieces"] >= 32 and lay["F"] >= 16, lay      # tens of pieces, several quads per key
    cols = [scalars(curve, n, 0x100 * log_n + 16 * m + j) for j in range(m)]
    cols[1][n // 2:] = 0                                           # fewer entries than the worst case: a finer cut
    run_guarded(h2, guarded, curve, bases_of(curve, n), cols)


def test_short_lists(h2, guarded):
    """only the first 300 scalars of a column are non-zero: ~ 30 entries per bucket in chunks of 8, so a key has 0 to a
    few pieces -- lists inside one chunk, lanes without a piece, piece counts that are no multiple of F"""
    curve, n, m = "pallas", 1 << 12, 3
    cols = [scalars(curve, n, 0x200 + j) for j in range(m)]
    for c in cols:
        c[300:] = 0
    run_guarded(h2, guarded, curve, bases_of(curve, n), cols)


@pytest.mark.parametrize("m", [3, 16])
@pytest.mark.parametrize("alternate", [False, True], ids=["same_point", "point_and_inverse"])
def test_exceptional_additions(h2, guarded, alternate, m):
    curve, n = "pallas", 1 << 12
    lay = layout(guarded, curve, n, m)
    cols = [scalars(curve, n, 0x300 + j) for j in range(m)]
    # no key is hot (those are summed by the task waves, tests/test_gpu_msm_front.py): the fullest bucket, cut into
    # chunks of at least 8 entries (the device's minimum), + 1 for a list that starts inside a chunk
    longest = max(longest_bucket_list(c, lay["c"], lay["W"]) for c in cols[:3])
    assert longest // 8 + 2 <= lay["hot_span"], (longest, lay)
    if m == 16:
        assert lay["pieces"] >= 2 * lay["F"], lay                  # several pieces per lane: stage 1 adds
    run_guarded(h2, guarded, curve, one_point_bases(curve, n, alternate), cols)


def test_workspace_reuse(h2):
    """no guard mode: its fill would hide what one launch sequence leaves behind for the next on the same workspace"""
    curve = "pallas"
    n, m = 1 << 12, 3
    b, other = bases_of(curve, n), bases_of(curve, 1 << 13)
    bases, big = h2.Bases(curve, b), h2.Bases(curve, other)
    try:
        cols = [scalars(curve, n, 0x400 + j) for j in range(m)]
        expect = [want(curve, c, b) for c in cols]
        got = bases.msm_batch(cols)
        for j in range(m):
            assert np.array_equal(got[j], expect[j]), j
        side = [scalars(curve, 1 << 13, 0x410 + j) for j in range(5)]
        got_side = big.msm_batch(side)                             # another shape, another F, on the same workspace
        for j in (0, 4):
            assert np.array_equal(got_side[j], want(curve, side[j], other)), ("side", j)
        again = bases.msm_batch(cols)
        for j in range(m):
            assert np.array_equal(again[j], expect[j]), ("repeat", j)
    finally:
        bases.release()
        big.release()
