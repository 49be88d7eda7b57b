"""The 29-bit working-form product of h2_field29.hpp (fe29_mul, fe29_sqr, fe29_mul_sub and the rounded-up fe29_mul_up)
against Python integers at the edges of its input bounds: limbs of magnitude 2^29 - 1 (2^30 - 1 for fe29_mul's first
operand) and operand values whose product is near +-64 p^2.  Checks the value mod p, the exact output interval
(X / R' - p, X / R'] of the subtractive reduction, the limb bounds and the exact output limbs of pyref's model.

* CPU: the host instantiation (h2_selftest_fe29_op); also products past 64 p^2 that stay within the limb bounds --
  the (+-32 p)^2 of expr_kernel and the (+-16 p)^2 of perm_ratio_kernel -- where only the exact value is promised.
* GPU: every operand set of the CPU tests through the device instantiation (h2_selftest_fe29_op_device: the
  fe29_opaque / fe29_hidden asm statements and v_mad_i64_i32 shape that compile), limbs equal to the host's and the
  model's bit for bit."""
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


def sqr_cases(f, rng):
    """fe29_sqr operands: limbs below 2^29, |a|^2 <= 64 p^2"""
    p = f.p
    cases = [edge(rng, s * t, 1 << 29) for s in (1, -1) for t in (8 * p - (1 << 234), 4 * p, p, 1 << 240)]
    cases += [[rng.randrange(-(1 << 29) + 1, 1 << 29) for _ in range(8)] + [rng.randrange(-(1 << 23), 1 << 23)]
              for _ in range(40)]
    cases += [normalised(p - 1), normalised(-(8 * p) + 1), [(1 << 29) - 1] * 8 + [0], [-(1 << 29) + 1] * 8 + [0]]
    return cases


def mul_sub_cases(f, rng):
    """fe29_mul_sub operands (a, b, c, d): limbs below 2^29, |a b - c d| <= 64 p^2"""
    p = f.p
    sets = operand_sets(f, rng, 1 << 29, 1 << 29)
    out = []
    for i, (a, b) in enumerate(sets):
        c, d = sets[(5 * i + 1) % len(sets)]
        for cc, dd in ((c, d), ([0] * 9, d), ([-v for v in a], b)):      # a b - (-a) b = 2 a b: near +-128 p^2 is out
            if abs(value(a) * value(b) - value(cc) * value(dd)) <= 64 * p * p:
                out.append((a, b, cc, dd))
    # the edge: a b and c d of opposite signs adding up to +-64 p^2
    for s in (1, -1):
        a, b = edge(rng, s * 4 * p, 1 << 29), edge(rng, 8 * p, 1 << 29)
        c, d = edge(rng, -s * 4 * p, 1 << 29), edge(rng, 8 * p, 1 << 29)
        if abs(value(a) * value(b) - value(c) * value(d)) <= 64 * p * p:
            out.append((a, b, c, d))
    return out


def beyond_sets(f, rng, lim_a, lim_b):
    """(a, b) past |a| |b| <= 64 p^2 but within the limb bounds: what the prover's kernels multiply -- (+-16 p)^2
    (perm_ratio_kernel), (+-32 p)^2 (expr_kernel, values up to EXPR_VALUE_BOUND p) and (+-64 p) (p - 1) (expr_kernel's
    reduction of a sum of up to 64 p by one); values at the edge and limbs at +-(lim - 1)"""
    p = f.p
    out = []
    for sa in (1, -1):
        for sb in (1, -1):
            for va, vb in ((16 * p, 16 * p), (32 * p, 32 * p), (64 * p, p - 1), (32 * p - 1, 16 * p + 1)):
                out.append((edge(rng, sa * va, lim_a), edge(rng, sb * vb, lim_b)))
    for sa in (1, -1):                      # the same values with normalised limbs
        out.append((normalised(sa * 64 * p), normalised(p - 1)))
        for va in (16 * p, 32 * p):
            out.append((normalised(sa * va), normalised(va)))
            out.append((normalised(sa * va), normalised(-va)))
    for _ in range(24):                     # random values between 64 p^2 and 1024 p^2, random limbs
        va, vb = rng.randrange(8 * p, 32 * p), rng.randrange(8 * p, 32 * p)
        out.append((edge(rng, rng.choice((1, -1)) * va, lim_a), edge(rng, rng.choice((1, -1)) * vb, lim_b)))
    for a, b in out:
        assert all(abs(v) < lim_a for v in a) and all(abs(v) < lim_b for v in b)
        assert abs(value(a)) * abs(value(b)) > 60 * p * p
    return out


def device_cases(f, fid):
    """every operand set the CPU tests run, per op, as the 36-limb rows the hooks take"""
    cases = {MUL: [], SQR: [], MUL_SUB: [], MUL_UP: []}
    zero = [0] * 9
    for a, b in operand_sets(f, random.Random(fid), 1 << 30, 1 << 29):
        cases[MUL] += [a + b + zero + zero, b + a + zero + zero]
        if value(a) >= 0 and value(b) >= 0:
            cases[MUL_UP].append(a + b + zero + zero)
    for a in sqr_cases(f, random.Random(100 + fid)):
        cases[SQR].append(a + zero * 3)
    for a, b, c, d in mul_sub_cases(f, random.Random(200 + fid)):
        cases[MUL_SUB].append(a + b + c + d)
    for a, b in beyond_sets(f, random.Random(300 + fid), 1 << 30, 1 << 29):
        cases[MUL] += [a + b + zero + zero, b + a + zero + zero]
        if value(a) >= 0 and value(b) >= 0:
            cases[MUL_UP].append(a + b + zero + zero)
    for a, b in beyond_sets(f, random.Random(400 + fid), 1 << 29, 1 << 29):
        if abs(value(a)) <= 33 * f.p:
            cases[SQR].append(a + zero * 3)
        cases[MUL_SUB].append(a + b + b + a)      # a b - b a = 0: exact cancellation of two big products
        cases[MUL_SUB].append(a + b + zero + zero)
    return cases


def model(f, op, row):
    a, b, c, d = (row[9 * k:9 * k + 9] for k in range(4))
    if op == SQR:
        return R.fe29_reduce(value(a) ** 2, f.p)
    if op == MUL_SUB:
        return R.fe29_reduce(value(a) * value(b) - value(c) * value(d), f.p)
    if op == MUL_UP:
        return R.fe29_reduce_up(value(a) * value(b), f.p)
    return R.fe29_reduce(value(a) * value(b), f.p)


def check(f, x, r, up=False, in_contract=True):
    """r = the product's limbs for the integer X = x; in_contract: |X| <= 64 p^2, where (-3p/2, p/2] is promised"""
    p = f.p
    assert all(0 <= v < (1 << L) for v in r[:8]), r
    assert abs(r[8]) < (1 << 26), r
    v = value(r)
    assert (v * RP - x) % p == 0
    assert r == (R.fe29_reduce_up(x, p) if up else R.fe29_reduce(x, p))     # the exact limbs
    if up:
        assert x <= v * RP < x + p * RP                    # (X + m p) / R' with 0 <= m < R'
        return
    assert x - p * RP < v * RP <= x                        # (X - m p) / R' with 0 <= m < R'
    if not in_contract:
        return
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
    p = f.p
    for a in sqr_cases(f, random.Random(100 + fid)):
        assert value(a) ** 2 <= 64 * p * p
        check(f, value(a) ** 2, run(lib, fid, SQR, a))


@pytest.mark.parametrize("name", list(R.FIELDS))
def test_fe29_mul_sub_at_the_bounds(lib, name):
    f, fid = R.FIELDS[name], O.FIELD_IDS[name]
    n = 0
    for a, b, c, d in mul_sub_cases(f, random.Random(200 + fid)):
        check(f, value(a) * value(b) - value(c) * value(d), run(lib, fid, MUL_SUB, a, b, c, d))
        n += 1
    assert n > 40


@pytest.mark.parametrize("name", list(R.FIELDS))
def test_fe29_mul_past_64p2_within_the_limb_bounds(lib, name):
    """products up to 1024 p^2: exact (X - m p) / R' (and the additive form's (X + m' p) / R'), no range promised"""
    f, fid = R.FIELDS[name], O.FIELD_IDS[name]
    n = 0
    for a, b in beyond_sets(f, random.Random(300 + fid), 1 << 30, 1 << 29):
        x = value(a) * value(b)
        check(f, x, run(lib, fid, MUL, a, b), in_contract=abs(x) <= 64 * f.p ** 2)
        check(f, x, run(lib, fid, MUL, b, a), in_contract=abs(x) <= 64 * f.p ** 2)
        if value(a) >= 0 and value(b) >= 0:
            check(f, x, run(lib, fid, MUL_UP, a, b), up=True)
        n += 1
    for a, b in beyond_sets(f, random.Random(400 + fid), 1 << 29, 1 << 29):
        if abs(value(a)) <= 33 * f.p:                   # squares up to the (32 p)^2 the callers reach
            check(f, value(a) ** 2, run(lib, fid, SQR, a), in_contract=False)
        check(f, 0, run(lib, fid, MUL_SUB, a, b, b, a))
        x = value(a) * value(b)
        check(f, x, run(lib, fid, MUL_SUB, a, b, [0] * 9, [0] * 9), in_contract=abs(x) <= 64 * f.p ** 2)
    assert n >= 40


def test_fe29_model_matches_the_host_hook_row_layout(lib):
    """device_cases' rows through the host hook give the model's limbs (the GPU test compares against both)"""
    f, fid = R.BN_FR, O.FIELD_IDS["bn254_fr"]
    for op, rows in device_cases(f, fid).items():
        assert rows
        for row in rows[:8] + rows[-8:]:
            assert run(lib, fid, op, *(row[9 * k:9 * k + 9] for k in range(4))) == model(f, op, row)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(R.FIELDS))
def test_gpu_fe29_ops_match_the_host_and_the_model_bit_for_bit(h2, name):
    """the device instantiation, one launch per op over every operand set of the CPU tests (old and past 64 p^2)"""
    lib = h2.load()
    f, fid = R.FIELDS[name], O.FIELD_IDS[name]
    for op, rows in device_cases(f, fid).items():
        buf = np.ascontiguousarray(np.array(rows, dtype=np.int64).astype(np.int32))
        assert buf.shape == (len(rows), 36)
        out = np.zeros((len(rows), 9), dtype=np.int32)
        assert lib.h2_selftest_fe29_op_device(fid, op, buf.ctypes.data_as(ctypes.c_void_p),
                                              out.ctypes.data_as(ctypes.c_void_p), len(rows)) == 0
        for i, row in enumerate(rows):
            want = model(f, op, row)
            host = run(lib, fid, op, *(row[9 * k:9 * k + 9] for k in range(4)))
            got = [int(v) for v in out[i]]
            assert got == host == want, (name, op, i)
