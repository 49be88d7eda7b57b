"""Operand sets for the working-form group law (h2_curve29.hpp, h2_curve_quad.hpp) over the whole range of a stored
coordinate, shared by tests/test_xyzz29_ranges.py (host instantiation) and tests/test_gpu_xyzz29_ranges.py (device).

TEST INFRASTRUCTURE ONLY, like pyref.  A case is built from curve points (P, Q) of pyref, scale factors lambda / mu
(x = X l^2, y = Y l^3, zz = l^2, zzz = l^3) and an integer representative per coordinate: the working form of a value v
is v 2^261 mod p plus k p, as fe29_normalised limbs, with k anywhere the stored-point contract admits:
x in (-3p, 5p), y in (-2p, 2p), zz and zzz in (-3p/2, p).  Everything is drawn from a fixed seed per curve."""
import collections
import functools
import random

import pyref as R

# the stored-point contract, in units of p / 2 (open intervals)
RANGE2 = {"x": (-6, 10), "y": (-4, 4), "zz": (-3, 2), "zzz": (-3, 2)}
COORDS = ("x", "y", "zz", "zzz")
ADD, DOUBLE, ADD_AFFINE, DOUBLE_AFFINE, ADD_QUAD, DOUBLE_QUAD, ADD_AFFINE_CHAIN, DOUBLE_AFFINE_CHAIN = range(8)
PROJECTIVE_OPS = (ADD, DOUBLE, ADD_QUAD, DOUBLE_QUAD)          # operand B is a stored point
AFFINE_OPS = (ADD_AFFINE, DOUBLE_AFFINE, ADD_AFFINE_CHAIN, DOUBLE_AFFINE_CHAIN)   # operand B is a table entry
CLASSES = ("generic", "doubling", "cancelling", "identity-in")

# row: the 72 limbs the hooks take; P, Q: the affine big-integer points the operands stand for (None = identity);
# edge: a canonical edge value (x or y in {1, p - 1}), kept out of the class counts
Case = collections.namedtuple("Case", "row P Q edge")


def admissible(c, coord, p):
    """every k with c + k p strictly inside the stored range of `coord` (c canonical)"""
    lo2, hi2 = RANGE2[coord]
    return [k for k in range(-4, 6) if lo2 * p < 2 * (c + k * p) < hi2 * p]


def working(v, p):
    """canonical value -> canonical working form"""
    return v * R.FE29_R % p


def representative(c, coord, how, p, rng):
    """limbs of c + k p: how = "lo" / "hi" (the lowest / highest admissible k), "rand", or k itself"""
    ks = admissible(c, coord, p)
    if how == "lo":
        k = ks[0]
    elif how == "hi":
        k = ks[-1]
    elif how == "rand":
        k = rng.choice(ks)
    else:
        k = how
        assert k in ks, (coord, k)
    return R.fe29_normalised(c + k * p)


def stored(curve, P, lam, hows, rng):
    """the 36 limbs of the stored point lam * P with the representatives `hows` = (x, y, zz, zzz).  The identity: zz
    exactly zero; its other coordinates mean nothing, so they are drawn inside their ranges too"""
    p = curve.base.p
    if P is None:
        junk = [representative(rng.randrange(p), c, "rand", p, rng) for c in COORDS]
        junk[2] = [0] * 9
        return sum(junk, [])
    l2 = lam * lam % p
    l3 = l2 * lam % p
    vals = (P[0] * l2 % p, P[1] * l3 % p, l2, l3)
    return sum((representative(working(v, p), c, how, p, rng) for v, c, how in zip(vals, COORDS, hows)), [])


def table_entry(curve, Q, negated):
    """the 18 limbs of an affine operand for the point Q: (x, y) canonical and unpacked, or -- `negated` -- what
    affine29_load(.., negate) makes of the table entry of -Q: y = the limb-wise negation of p - Q.y"""
    p = curve.base.p
    if Q is None:
        return [0] * 18
    x = R.fe29_unpack(working(Q[0], p))
    if negated:
        return x + R.fe29_neg(R.fe29_unpack(working(p - Q[1], p)))
    return x + R.fe29_unpack(working(Q[1], p))


def cube_root(a, p):
    """a cube root of a mod p where one of the closed forms applies, else None"""
    a %= p
    for e in ((2 * p - 1) // 3 if p % 3 == 2 else None, (2 * p + 1) // 9 if p % 9 == 4 else None,
              (p + 2) // 9 if p % 9 == 7 else None):
        if e is not None:
            r = pow(a, e, p)
            if r * r * r % p == a:
                return r
    return None


def edge_points(curve):
    """curve points with x or y in {1, p - 1}, as API values and as working-form values, where they exist"""
    f, p, b = curve.base, curve.base.p, curve.b
    rinv = pow(R.FE29_R, -1, p)
    out = []
    for v in (1, p - 1, rinv, p - rinv):
        y = f.sqrt((v * v * v + b) % p)
        if y is not None and y != 0:
            out.append((v, y))
        x = cube_root(v * v - b, p)
        if x is not None:
            out.append((x, v))
    assert all(curve.is_on_curve(P) for P in out)
    return out


def classify(curve, op, P, Q):
    """with big integers only: which branch of the formula the operands ask for"""
    if op in (DOUBLE, DOUBLE_QUAD):
        return "identity-in" if P is None else "doubling"
    if op in (DOUBLE_AFFINE, DOUBLE_AFFINE_CHAIN):
        return "identity-in" if Q is None else "doubling"
    if P is None or Q is None:
        return "identity-in"
    if P == Q:
        return "doubling"
    if P == curve.neg(Q):
        return "cancelling"
    return "generic"


def expected(curve, op, P, Q):
    if op in (DOUBLE, DOUBLE_QUAD):
        return curve.add(P, P)
    if op in (DOUBLE_AFFINE, DOUBLE_AFFINE_CHAIN):
        return curve.add(Q, Q)
    return curve.add(P, Q)


def applicable_classes(op):
    return ("doubling", "identity-in") if op in (DOUBLE, DOUBLE_QUAD, DOUBLE_AFFINE, DOUBLE_AFFINE_CHAIN) else CLASSES


Cases = collections.namedtuple("Cases", "projective affine")


@functools.lru_cache(maxsize=None)
def cases(name):
    """(projective, affine): the Case lists for ops whose operand B is a stored point / a table entry"""
    curve = R.CURVES[name]
    p = curve.base.p
    rng = random.Random(0x29C0 + curve.cid)
    pool = [curve.mul(rng.randrange(1, curve.scalar.p), curve.gen) for _ in range(12)]
    P0, Q0 = pool[0], pool[1]
    ONE = (0, 0)                                   # k of zz, zzz for lambda = 1: the canonical one of xyzz29_from_affine

    def scales():
        """(lambda, mu): 1 and 1; different; the same class (lambda = mu), different representatives only"""
        lam, mu = rng.randrange(2, p), rng.randrange(2, p)
        return ((1, 1), (lam, mu), (lam, lam))

    def hows4(lam, pick):
        """representatives for (x, y, zz, zzz); zz and zzz stay the canonical one when lambda = 1"""
        h = [pick(), pick(), pick(), pick()]
        return tuple(h[:2]) + ONE if lam == 1 else tuple(h)

    proj, aff = [], []

    def add_proj(P, lam, ha, Q, mu, hb, edge=False):
        proj.append(Case(stored(curve, P, lam, ha, rng) + stored(curve, Q, mu, hb, rng), P, Q, edge))

    def add_aff(P, lam, ha, Q, edge=False):
        a = stored(curve, P, lam, ha, rng)
        for negated in (False, True):
            aff.append(Case(a + table_entry(curve, Q, negated) + [0] * 18, P, Q, edge))

    rand3 = lambda: rng.choice(("lo", "hi", "rand"))

    # ---- Q unrelated to P: every coordinate at the low edge, the high edge or a random representative --------------------
    lam, mu = rng.randrange(2, p), rng.randrange(2, p)
    for bits in range(256):                                            # all 2^8 low / high combinations of one pair
        h = ["hi" if bits >> i & 1 else "lo" for i in range(8)]
        add_proj(P0, lam, tuple(h[:4]), Q0, mu, tuple(h[4:]))
    for bits in range(16):
        add_aff(P0, lam, tuple("hi" if bits >> i & 1 else "lo" for i in range(4)), Q0)
    for i in range(320):
        P, Q = rng.sample(pool, 2)
        lam, mu = scales()[i % 3]
        add_proj(P, lam, hows4(lam, rand3), Q, mu, hows4(mu, rand3))
        if i < 200:
            add_aff(P, lam, hows4(lam, rand3), Q)

    # ---- Q = P and Q = -P: every admissible k of x and of y on one operand, the other at random ---------------------------
    for sign in (1, -1):
        for P in (pool[2], pool[3]):
            Q = P if sign == 1 else curve.neg(P)
            for lam, mu in scales():
                l2, l3 = lam * lam % p, lam * lam * lam % p
                m2, m3 = mu * mu % p, mu * mu * mu % p
                for kx in admissible(working(P[0] * l2 % p, p), "x", p):
                    for ky in admissible(working(P[1] * l3 % p, p), "y", p):
                        swept = (kx, ky) + (ONE if lam == 1 else (rand3(), rand3()))
                        add_proj(P, lam, swept, Q, mu, hows4(mu, rand3))
                        add_aff(P, lam, swept, Q)
                for kx in admissible(working(Q[0] * m2 % p, p), "x", p):
                    for ky in admissible(working(Q[1] * m3 % p, p), "y", p):
                        swept = (kx, ky) + (ONE if mu == 1 else (rand3(), rand3()))
                        add_proj(P, lam, hows4(lam, rand3), Q, mu, swept)

    # ---- Q = +-P where the two sides of a difference get DIFFERENT representatives -----------------------------------------
    # A product's result is (a b - m p) / R' in (a b / R' - p, a b / R']: for a canonical value c it is c - p unless
    # a b / R' >= c, which takes a small c and two large operands of one sign.  Scale factors are searched for so that the
    # highest representatives reach that on either side; the low / high combinations then give u2 - u1 (s2 - s1) = -p, 0
    # and p, and u2 - acc.x = 3 p with acc.x at its lowest representative
    def top(v, coord):
        c = working(v % p, p)
        return c + admissible(c, coord, p)[-1] * p

    def search(cond):
        while True:
            lam, mu = rng.randrange(2, p), rng.randrange(2, p)
            if cond(lam, mu):
                return lam, mu

    P = pool[4]
    for coord, power, zcoord in (("x", 2, "zz"), ("y", 3, "zzz")):
        v = P[0] if coord == "x" else P[1]
        lam, mu = search(lambda l, m: min(top(v * pow(l, power, p), coord) * top(pow(m, power, p), zcoord),
                                          top(v * pow(m, power, p), coord) * top(pow(l, power, p), zcoord))
                         >= working(v * pow(l * m, power, p) % p, p) * R.FE29_R)
        for Q in (P, curve.neg(P)):
            for bits in range(256):
                h = ["hi" if bits >> i & 1 else "lo" for i in range(8)]
                add_proj(P, lam, tuple(h[:4]), Q, mu, tuple(h[4:]))
    lam, _ = search(lambda l, m: working(P[0], p) * top(l * l, "zz") >= working(P[0] * l * l % p, p) * R.FE29_R)
    for Q in (P, curve.neg(P)):
        for kx in admissible(working(P[0] * lam * lam % p, p), "x", p):
            for ky in admissible(working(P[1] * pow(lam, 3, p) % p, p), "y", p):
                for hz in ("lo", "hi"):
                    add_aff(P, lam, (kx, ky, hz, rand3()), Q)

    # ---- identity operands: A, B, both; the table's (0, 0) entry ---------------------------------------------------------
    zero_identity = [0] * 36
    for i in range(8):
        P, Q = rng.sample(pool, 2)
        lam, mu = scales()[i % 3]
        add_proj(None, 1, None, Q, mu, hows4(mu, rand3))
        add_proj(P, lam, hows4(lam, rand3), None, 1, None)
        add_proj(None, 1, None, None, 1, None)
        add_aff(None, 1, None, Q)
        add_aff(P, lam, hows4(lam, rand3), None)
        add_aff(None, 1, None, None)
    b = stored(curve, Q0, 1, ("rand", "rand", 0, 0), rng)
    proj += [Case(zero_identity + b, None, Q0, False), Case(b + zero_identity, Q0, None, False),
             Case(zero_identity + zero_identity, None, None, False)]
    aff += [Case(zero_identity + table_entry(curve, Q0, False) + [0] * 18, None, Q0, False),
            Case(zero_identity + [0] * 36, None, None, False)]

    # ---- a curve point with x = 0: the coordinate is exactly zero, the point is not the identity -------------------------
    y0 = curve.base.sqrt(curve.b)
    if y0:
        for Z in ((0, y0), (0, p - y0)):
            for lam, mu in scales():
                for other in (Q0, Z, curve.neg(Z)):
                    for kx in admissible(0, "x", p):
                        hz = (kx, rand3()) + (ONE if lam == 1 else (rand3(), rand3()))
                        add_proj(Z, lam, hz, other, mu, hows4(mu, rand3))
                        add_proj(other, mu, hows4(mu, rand3), Z, lam, hz)
                        add_aff(Z, lam, hz, other)
                    add_aff(other, mu, hows4(mu, rand3), Z)

    # ---- canonical edge values (not counted in the classes) --------------------------------------------------------------
    for E in edge_points(curve):
        for other in (Q0, E, curve.neg(E)):
            lam, mu = scales()[1]
            add_proj(E, 1, ("rand", "rand", 0, 0), other, mu, hows4(mu, rand3), edge=True)
            add_proj(other, mu, hows4(mu, rand3), E, 1, (0, 0, 0, 0), edge=True)
            add_aff(other, mu, hows4(mu, rand3), E, edge=True)
            add_aff(E, 1, (0, 0, 0, 0), other, edge=True)
    return Cases(proj, aff)


def cases_of(name, op):
    c = cases(name)
    return c.projective if op in PROJECTIVE_OPS else c.affine


MODELS = {ADD: R.xyzz29_add, ADD_QUAD: R.xyzz29_add_quad}


def split(row):
    """72 limbs -> (A, B), each (x, y, zz, zzz)"""
    return tuple(tuple(row[36 * h + 9 * c:36 * h + 9 * c + 9] for c in range(4)) for h in range(2))


def model_row(name, op, row, chk=None):
    """the 36 limbs pyref's model gives for one row"""
    p = R.CURVES[name].base.p
    A, B = split(row)
    if op in (ADD, ADD_QUAD):
        r = MODELS[op](A, B, p, chk)
    elif op == DOUBLE:
        r = R.xyzz29_double(A, p, chk)
    elif op == DOUBLE_QUAD:
        r = R.xyzz29_double_quad(A, p, chk)
    elif op in (ADD_AFFINE, ADD_AFFINE_CHAIN):
        r = R.xyzz29_add_affine(A, B[:2], p, chk)
    else:
        r = R.xyzz29_double_affine(B[:2], p, chk)
    return [int(v) for c in r for v in c]


@functools.lru_cache(maxsize=None)
def modelled(name, op):
    """(outputs, check): the model's limbs for every case of `op` in the checking mode, and the Fe29Check that followed
    them.  Raises where the model's own preconditions break"""
    chk = R.Fe29Check(R.CURVES[name].base.p)
    return [model_row(name, op, c.row, chk) for c in cases_of(name, op)], chk


def _rows_buffer(rows):
    import numpy as np
    buf = np.ascontiguousarray(np.array(rows, dtype=np.int64).astype(np.int32))
    assert buf.shape == (len(rows), 72)
    return np, buf


def host_rows(lib, cid, op, rows):
    """every row through h2_selftest_xyzz29_op (ops 0..3) -> (n, 36) int32"""
    np, buf = _rows_buffer(rows)
    out = np.zeros((len(rows), 36), dtype=np.int32)
    for i in range(len(rows)):
        assert lib.h2_selftest_xyzz29_op(cid, op, buf[i].ctypes.data, out[i].ctypes.data) == 0
    return out


def device_rows(lib, cid, op, rows):
    """every row through h2_selftest_xyzz29_op_device in one launch -> (n, 4, 36) int32, one copy per lane of the quad"""
    np, buf = _rows_buffer(rows)
    out = np.zeros((len(rows), 4, 36), dtype=np.int32)
    assert lib.h2_selftest_xyzz29_op_device(cid, op, buf.ctypes.data, out.ctypes.data, len(rows)) == 0
    return out


def class_counts(name, op):
    curve = R.CURVES[name]
    n = collections.Counter(classify(curve, op, c.P, c.Q) for c in cases_of(name, op) if not c.edge)
    return {k: n.get(k, 0) for k in applicable_classes(op)}


def check_result(curve, out, want, y_range2=(-4, 4)):
    """`out` (36 limbs) is a stored point inside the contract that stands for the affine point `want`, by big integers
    only: limbs normalised, every coordinate strictly inside its range, x = X zz, y = Y zzz, zz^3 = zzz^2, zz != 0.
    The identity is judged by zz exactly zero and nothing else of it is looked at.  Returns None or what is wrong"""
    p = curve.base.p
    co = [out[9 * i:9 * i + 9] for i in range(4)]
    if not any(co[2]):
        return None if want is None else "identity returned for a finite point"
    if want is None:
        return "a finite point returned for the identity"
    for c, limbs in zip(COORDS, co):
        if not all(0 <= v < (1 << 29) for v in limbs[:8]):
            return c + ": limbs not normalised"
        lo2, hi2 = y_range2 if c == "y" else RANGE2[c]
        if not lo2 * p < 2 * R.fe29_value(limbs) < hi2 * p:
            return c + ": outside the stored range (%.3f p)" % (R.fe29_value(limbs) / p)
    rinv = pow(R.FE29_R, -1, p)
    x, y, zz, zzz = (R.fe29_value(limbs) * rinv % p for limbs in co)
    if zz == 0 or zzz == 0:
        return "zz or zzz is zero mod p"
    if (zz * zz * zz - zzz * zzz) % p:
        return "zz^3 != zzz^2"
    if (x - want[0] * zz) % p or (y - want[1] * zzz) % p:
        return "not the expected point"
    return None
