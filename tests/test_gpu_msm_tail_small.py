"""GPU: the three tail kernels of the MSM (fix-up, row / column sums, final) end to end at their smallest shapes, on
the four-lanes-per-point operations of csrc/h2_curve_quad.hpp: n = 2^10 and 2^12 terms in launches of m = 1, 3, 4, 5
columns (the column counts of the prover's launch sequences, and the lone column) in guard mode against the CPU oracle,
and one launch with a column of equal scalars, whose buckets are summed by the fix-up's task waves (the quad addition
in a loop and the shuffle tree on the hot path)."""
import ctypes

import numpy as np
import pytest

import oracle_lib as O
import pyref as R

pytestmark = pytest.mark.gpu
SEED = 0x48324D5351440000
CURVE = "pallas"
CID = O.CURVE_IDS[CURVE]
_SHARED = {}


def scalars(n, seed):
    return O.synth_scalars(O.CURVE_SCALAR_FIELD[CID], SEED | seed, n).reshape(n, 4)


def shared(log_n):
    """(bases, five columns, their commitments by the oracle) of one size, computed once and never modified"""
    if log_n not in _SHARED:
        n = 1 << log_n
        b = O.synth_bases(CID, SEED | 0xB7, n, threads=8).reshape(n, 8)
        cols = [scalars(n, 0x100 * log_n + j) for j in range(5)]
        cols[1][n // 2:] = 0
        expect = [O.to_affine(CID, O.best_multiexp(CID, np.ascontiguousarray(c), np.ascontiguousarray(b), threads=8)) for c in cols]
        for a in [b] + cols + expect:
            a.setflags(write=False)
        _SHARED[log_n] = (b, cols, expect)
    return _SHARED[log_n]


def guard_report(lib):
    out = (ctypes.c_uint64 * 2)()
    first = ctypes.create_string_buffer(256)
    assert lib.h2_selftest_msm_guard_report(out, first, 256) == 0
    return int(out[0]), int(out[1]), first.value.decode()


@pytest.fixture()
def guarded(h2):
    lib = h2.load()
    lib.h2_selftest_msm_guard(1)
    yield lib
    lib.h2_selftest_msm_guard(0)


@pytest.mark.parametrize("m", [1, 3, 4, 5])
@pytest.mark.parametrize("log_n", [10, 12])
def test_small_launches_against_the_oracle(h2, guarded, log_n, m):
    b, cols, expect = shared(log_n)
    bases = h2.Bases(CURVE, b)
    try:
        got = bases.msm_batch(cols[:m])
        launches, violations, first = guard_report(guarded)
        assert launches >= 1 and violations == 0, first
        for j in range(m):
            assert np.array_equal(got[j], expect[j]), j
    finally:
        bases.release()


def test_a_column_of_equal_scalars_runs_the_task_waves(h2):
    lib = h2.load()
    log_n, m = 12, 3
    n = 1 << log_n
    front = (ctypes.c_uint64 * 12)()
    assert lib.h2_selftest_msm_front(CID, n, n, m, 1, front) == 0
    T, hot_span, hot_seg, max_tasks = (int(front[i]) for i in (8, 9, 10, 11))
    pieces = -(-n // T)                      # a non-zero window's n entries in one bucket: at least this many pieces
    assert pieces > hot_span and 0 < -(-pieces // hot_seg) <= max_tasks, (T, hot_span, hot_seg, max_tasks)
    b, cols, expect = shared(log_n)
    const = np.tile(np.array(R.CURVES[CURVE].scalar.limbs(0x1234567ABCDEF << 150 | 0x6F3A59C1), dtype=np.uint64), (n, 1))
    bases = h2.Bases(CURVE, b)
    try:
        got = bases.msm_batch([const, cols[0], cols[1]])
        assert np.array_equal(got[0], O.to_affine(CID, O.best_multiexp(CID, const, np.ascontiguousarray(b), threads=8)))
        assert np.array_equal(got[1], expect[0]) and np.array_equal(got[2], expect[1])
    finally:
        bases.release()
