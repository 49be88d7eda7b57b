"""GPU: the single-chain form of the 29-bit Montgomery product (csrc/h2_field29_chain.hpp) against the compiler's form
(csrc/h2_field29.hpp) -- the nine output limbs must be EQUAL, not merely congruent: the chain is the same integer
operations modulo 2^64, one v_mad_i64_i32 per limb product with the accumulator as its addend.

h2_selftest_fe29_chain_device runs op in {mul, sqr, mul_sub, mul_up} on n operand tuples given as raw limbs through both
device forms and returns both sets of limbs.  Both Pasta fields (the chain exists where p = 1 mod 2^29), 4096 random
tuples per op plus a fixed edge list; the compiler's side of every tuple is also checked against Python integers, as
tests/test_fe29_product.py does for the host instantiation.
"""
import ctypes
import random

import numpy as np
import pytest

import oracle_lib as O
import pyref as R

L = 29
LIM = 1 << 29
MUL, SQR, MUL_SUB, MUL_UP = 0, 1, 2, 3
OPS = {MUL: "mul", SQR: "sqr", MUL_SUB: "mul_sub", MUL_UP: "mul_up"}
PASTA = ["pasta_fp", "pasta_fq"]
N_RANDOM = 4096


def value(limbs):
    return sum(int(v) << (L * i) for i, v in enumerate(limbs))


def normalised(x):
    """signed integer -> limbs 0..7 in [0, 2^29), the top limb signed"""
    return [(x >> (L * i)) & (LIM - 1) for i in range(8)] + [x >> (8 * L)]


def edge_rows(p, op):
    """36-limb rows (a, b, c, d) at the edges of the op's limb bounds.  Only the limb bounds matter for the equality of
    the two forms (and for the exact model): sums of 18 limb products and nine m p terms stay below 2^63."""
    hi, lo = [LIM - 1] * 9, [-(LIM - 1)] * 9
    hi30, lo30 = [2 * LIM - 1] * 9, [-(2 * LIM - 1)] * 9          # fe29_mul allows one operand up to 2^30 - 1
    zero, one, pm1 = [0] * 9, normalised(1), normalised(p - 1)
    alt = [(LIM - 1) * (-1) ** i for i in range(9)]
    singles = [hi, lo, zero, one, pm1, alt, normalised(-(p - 1)), normalised(p)]
    rows = []
    if op == SQR:
        return [a + zero * 3 for a in singles]
    if op in (MUL, MUL_UP):
        for a in singles:
            for b in singles:
                rows.append(a + b + zero * 2)
        for a in (hi30, lo30):                                   # the 2^30 side, against every 2^29 operand, both orders
            for b in singles:
                rows.append(a + b + zero * 2)
                rows.append(b + a + zero * 2)
        return rows
    # mul_sub: a b - c d; the column sums reach the bound of 18 limb products when -c d has the sign of a b
    for a in singles:
        for b in singles:
            rows.append(a + b + zero + zero)
            rows.append(a + b + b + a)                           # exact cancellation
    for a, b, c, d in ((hi, hi, lo, hi), (hi, hi, hi, lo), (lo, lo, hi, lo), (hi, lo, hi, hi), (lo, hi, lo, lo),
                       (hi, hi, hi, hi), (alt, alt, [-v for v in alt], alt), (pm1, pm1, pm1, one)):
        rows.append(a + b + c + d)
    return rows


def random_rows(op, seed):
    rng = np.random.default_rng(seed)
    rows = rng.integers(-(LIM - 1), LIM, size=(N_RANDOM, 36), dtype=np.int64)
    if op in (MUL, MUL_UP):
        rows[: N_RANDOM // 2, :9] = rng.integers(-(2 * LIM - 1), 2 * LIM, size=(N_RANDOM // 2, 9), dtype=np.int64)
    return rows


def model(p, op, row):
    a, b, c, d = (row[9 * k:9 * k + 9] for k in range(4))
    if op == SQR:
        return R.fe29_reduce(value(a) ** 2, p)
    if op == MUL_SUB:
        return R.fe29_reduce(value(a) * value(b) - value(c) * value(d), p)
    if op == MUL_UP:
        return R.fe29_reduce_up(value(a) * value(b), p)
    return R.fe29_reduce(value(a) * value(b), p)


@pytest.mark.gpu
@pytest.mark.parametrize("op", list(OPS), ids=list(OPS.values()))
@pytest.mark.parametrize("name", PASTA)
def test_chain_form_returns_the_limbs_of_the_compilers_form(h2, name, op):
    lib = h2.load()
    f, fid = R.FIELDS[name], O.FIELD_IDS[name]
    edges = np.array(edge_rows(f.p, op), dtype=np.int64)
    rows = np.concatenate([edges, random_rows(op, 1000 * fid + op)])
    buf = np.ascontiguousarray(rows.astype(np.int32))
    n = buf.shape[0]
    assert n >= N_RANDOM + 8
    cpp = np.full((n, 9), -1, dtype=np.int32)
    chain = np.full((n, 9), -2, dtype=np.int32)
    assert lib.h2_selftest_fe29_chain_device(fid, op, buf.ctypes.data_as(ctypes.c_void_p), cpp.ctypes.data_as(ctypes.c_void_p),
                                             chain.ctypes.data_as(ctypes.c_void_p), n) == 0
    bad = np.nonzero((cpp != chain).any(axis=1))[0]
    assert bad.size == 0, (name, OPS[op], int(bad[0]), rows[bad[0]].tolist(), cpp[bad[0]].tolist(), chain[bad[0]].tolist())
    # the compiler's side against Python integers: every edge row and a stride through the random ones
    rng = random.Random(fid)
    picks = list(range(len(edges))) + [rng.randrange(len(edges), n) for _ in range(256)]
    for i in picks:
        assert [int(v) for v in cpp[i]] == model(f.p, op, [int(v) for v in rows[i]]), (name, OPS[op], i)


@pytest.mark.gpu
def test_chain_hook_refuses_the_fields_without_a_chain_form(h2):
    lib = h2.load()
    buf = np.zeros((1, 36), dtype=np.int32)
    out = np.zeros((2, 9), dtype=np.int32)
    for fid in (0, 1):                                           # BN254: dense modulus, p != 1 mod 2^29
        assert lib.h2_selftest_fe29_chain_device(fid, MUL, buf.ctypes.data_as(ctypes.c_void_p),
                                                 out[0].ctypes.data_as(ctypes.c_void_p),
                                                 out[1].ctypes.data_as(ctypes.c_void_p), 1) == -1
