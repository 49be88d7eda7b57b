"""CPU (no GPU): the 29-bit working-form product of h2_field29.hpp (fe29_mul, fe29_sqr, fe29_mul_sub and the
rounded-up fe29_mul_up), instantiated on the host, against Python integers at the edges of its documented input bounds:
limbs of magnitude 2^29 - 1 (2^30 - 1 for fe29_mul's first operand) and operand values whose product is near +-64 p^2.
Checks the value mod p, the exact output interval (X / R' - p, X / R'] of the subtractive reduction and the limb bounds."""
import ctypes
import random

import numpy as np
import pytest

import oracle_lib as O
import pyref as R

RP = 1 << 261              # R' of the working form
L = 29
MUL, SQR, MUL_SUB, MUL_UP = 0, 1, 2, 3


@pytest.fixture(scope="module")
def lib():
    import halo2_prover_amd
    return halo2_prover_amd.load()


def value(limbs):
    return sum(int(v) << (L * i) for i, v in enumerate(limbs))


def run(lib, fid, op, *operands):
    buf = np.zeros(36, dtype=np.int32)
    for k, x in enumerate(operands):
        buf[9 * k:9 * k + 9] = x
    out = np.zeros(9, dtype=np.int32)
    assert lib.h2_selftest_fe29_op(fid, op, buf.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p)) == 0
    return [int(v) for v in out]


def edge(rng, target, lim):
    """9 limbs of magnitude < lim whose low eight are at +-(lim - 1), the top limb chosen so the value is close to
    `target` (within 2^233)"""
    limbs = [rng.choice((-1, 1)) * (lim - 1) for _ in range(8)]
    low = value(limbs)
    top = (target - low) >> (8 * L)
    return limbs + [top]


def normalised(x):
    """signed integer -> limbs 0..7 in [0, 2^29), the top limb signed"""
    limbs = [(x >> (L * i)) & ((1 << L) - 1) for i in range(8)]
    return limbs + [x >> (8 * L)]


def operand_sets(f, rng, lim_a, lim_b):
    """(a, b) limb vectors with |a| |b| <= 64 p^2 at the limb and value edges"""
    p = f.p
    out = []
    for sa in (1, -1):
        for sb in (1, -1):
            for va, vb in ((8 * p, 8 * p), (64 * p, p - 1), (p // 2, 100 * p), (1 << 200, 8 * p)):
                a = edge(rng, sa * va, lim_a)
                b = edge(rng, sb * vb, lim_b)
                while abs(value(a)) * abs(value(b)) > 64 * p * p:      # pull the value that overshoots back in
                    a[8] -= 1 if value(a) > 0 else -1
                out.append((a, b))
    for _ in range(40):
        a = [rng.randrange(-lim_a + 1, lim_a) for _ in range(9)]
        b = [rng.randrange(-lim_b + 1, lim_b) for _ in range(9)]
        a[8] = rng.randrange(-(1 << 24), 1 << 24)
        b[8] = rng.randrange(-(1 << 24), 1 << 24)
        if abs(value(a)) * abs(value(b)) <= 64 * p * p:
            out.append((a, b))
    out.append((normalised(p - 1), normalised(p - 1)))
    out.append((normalised(-(p - 1)), normalised(p - 1)))
    out.append(([0] * 9, edge(rng, 8 * p, lim_b)))
    return out


def check(f, x, r, up=False):
    p = f.p
    assert all(0 <= v < (1 << L) for v in r[:8]), r
    assert abs(r[8]) < (1 << 26), r
    v = value(r)
    assert (v * RP - x) % p == 0
    if up:
        assert x <= v * RP < x + p * RP                    # (X + m p) / R' with 0 <= m < R'
        return
    assert x - p * RP < v * RP <= x                        # (X - m p) / R' with 0 <= m < R'
    # the documented range, (-3p/2, p/2] to within p 2^-127 (the Pasta primes exceed 2^254 slightly)
    assert -3 * p // 2 - (p >> 127) < v <= p // 2 + (p >> 127)


@pytest.mark.parametrize("name", list(R.FIELDS))
def test_fe29_mul_at_the_bounds(lib, name):
    f, fid = R.FIELDS[name], O.FIELD_IDS[name]
    rng = random.Random(fid)
    for a, b in operand_sets(f, rng, 1 << 30, 1 << 29):
        check(f, value(a) * value(b), run(lib, fid, MUL, a, b))
        check(f, value(b) * value(a), run(lib, fid, MUL, b, a))
        if value(a) >= 0 and value(b) >= 0:
            check(f, value(a) * value(b), run(lib, fid, MUL_UP, a, b), up=True)


@pytest.mark.parametrize("name", list(R.FIELDS))
def test_fe29_sqr_at_the_bounds(lib, name):
    f, fid = R.FIELDS[name], O.FIELD_IDS[name]
    rng = random.Random(100 + fid)
    p = f.p
    cases = [edge(rng, s * t, 1 << 29) for s in (1, -1) for t in (8 * p - (1 << 234), 4 * p, p, 1 << 240)]
    cases += [[rng.randrange(-(1 << 29) + 1, 1 << 29) for _ in range(8)] + [rng.randrange(-(1 << 23), 1 << 23)]
              for _ in range(40)]
    cases += [normalised(p - 1), normalised(-(8 * p) + 1), [(1 << 29) - 1] * 8 + [0], [-(1 << 29) + 1] * 8 + [0]]
    for a in cases:
        assert value(a) ** 2 <= 64 * p * p
        check(f, value(a) ** 2, run(lib, fid, SQR, a))


@pytest.mark.parametrize("name", list(R.FIELDS))
def test_fe29_mul_sub_at_the_bounds(lib, name):
    f, fid = R.FIELDS[name], O.FIELD_IDS[name]
    rng = random.Random(200 + fid)
    p = f.p
    sets = operand_sets(f, rng, 1 << 29, 1 << 29)
    n = 0
    for i, (a, b) in enumerate(sets):
        c, d = sets[(5 * i + 1) % len(sets)]
        for cc, dd in ((c, d), ([0] * 9, d), ([-v for v in a], b)):      # a b - (-a) b = 2 a b: near +-128 p^2 is out
            x = value(a) * value(b) - value(cc) * value(dd)
            if abs(x) > 64 * p * p:
                continue
            check(f, x, run(lib, fid, MUL_SUB, a, b, cc, dd))
            n += 1
    # the edge: a b and c d of opposite signs adding up to +-64 p^2
    for s in (1, -1):
        a, b = edge(rng, s * 4 * p, 1 << 29), edge(rng, 8 * p, 1 << 29)
        c, d = edge(rng, -s * 4 * p, 1 << 29), edge(rng, 8 * p, 1 << 29)
        x = value(a) * value(b) - value(c) * value(d)
        if abs(x) <= 64 * p * p:
            check(f, x, run(lib, fid, MUL_SUB, a, b, c, d))
            n += 1
    assert n > 40
