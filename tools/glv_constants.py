#!/usr/bin/env python3
"""Derive the GLV constants of the three curves and write halo2_prover_amd/csrc/h2_glv_constants.inc.

BN254, Pallas and Vesta are y^2 = x^3 + b with q = r = 1 (mod 3): phi(x, y) = (beta x, y) is an endomorphism,
phi(P) = [lambda] P with lambda^3 = 1 in the scalar field and beta^3 = 1 in the base field.  A scalar k splits as
k = k1 + k2 lambda (mod r) with short k1, k2 (the group FFT's twiddle multiplication, csrc/h2_group_fft.hpp).

Per curve:
  lambda, beta   paired so that (beta x, y) = [lambda](x, y) -- CHECKED below on the curve's generator against the
                 CPU oracle's scalar multiplication (each field has two primitive cube roots; the wrong pairing is
                 the other root, lambda^2)
  (a1, b1), (a2, b2)   a reduced basis of the lattice {(a, b) : a + b lambda = 0 mod r} (Lagrange-Gauss reduction)
  g1, g2         round(2^256 |b2| / r), round(2^256 |b1| / r): c_i = floor(k g_i / 2^256) approximates the magnitudes of
                 the coordinates k b2 / det, -k b1 / det of (k, 0) in that basis (det = a1 b2 - a2 b1 = +-r); their
                 signs s_i are folded into the constants the routine multiplies by
and then k1 = k - s1 c1 a1 - s2 c2 a2, k2 = -s1 c1 b1 - s2 c2 b2.  The congruence k1 + k2 lambda = k holds for ANY integers
c1, c2; only the size of k1, k2 depends on how well c_i approximates.  bound() below derives GLV_BITS from the
basis and the error of the floor, tests/test_glv_split.py checks it on the compiled routine.

Pure Python big integers; the only outside code is the oracle's scalar_mul for the pairing check.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import pyref as R  # noqa: E402

CURVE_ORDER = ["bn254", "pallas", "vesta"]
M256 = (1 << 256) - 1


def cube_root_of_unity(f):
    """a primitive cube root of unity of the field: gen^((p - 1) / 3)"""
    assert f.p % 3 == 1
    w = pow(f.gen, (f.p - 1) // 3, f.p)
    assert w != 1 and pow(w, 3, f.p) == 1 and (w * w + w + 1) % f.p == 0
    return w


def reduced_basis(r, lam):
    """Lagrange-Gauss reduction of the lattice spanned by (r, 0) and (-lambda, 1)"""
    u, v = (r, 0), ((-lam) % r, 1)

    def n2(w):
        return w[0] * w[0] + w[1] * w[1]
    if n2(u) < n2(v):
        u, v = v, u
    while True:
        # nearest integer to <u, v> / <v, v>
        num, den = u[0] * v[0] + u[1] * v[1], n2(v)
        m = (2 * num + den) // (2 * den)
        u = (u[0] - m * v[0], u[1] - m * v[1])
        if n2(u) >= n2(v):
            break
        u, v = v, u
    for w in (u, v):
        assert (w[0] + w[1] * lam) % r == 0
    return v, u


def derive(curve_name, check_pairing=True):
    c = R.CURVES[curve_name]
    r, q = c.scalar.p, c.base.p
    lam, beta = cube_root_of_unity(c.scalar), cube_root_of_unity(c.base)
    if check_pairing:
        import oracle_lib as O
        import numpy as np
        cid = O.CURVE_IDS[curve_name]
        gx, gy = c.gen
        aff = np.array(c.base.limbs(gx) + c.base.limbs(gy), dtype=np.uint64)

        def lam_times_g(l):
            out = O.to_affine(cid, O.scalar_mul(cid, np.array(c.scalar.limbs(l), dtype=np.uint64), aff))
            return (c.base.from_mont(O.limbs_to_int(out[:4])), c.base.from_mont(O.limbs_to_int(out[4:])))
        if lam_times_g(lam) != (beta * gx % q, gy):
            lam = lam * lam % r                                  # the other primitive root
        assert lam_times_g(lam) == (beta * gx % q, gy), "no cube root pairs with beta on " + curve_name
    (a1, b1), (a2, b2) = reduced_basis(r, lam)
    det = a1 * b2 - a2 * b1
    assert abs(det) == r
    # (k, 0) = x1 v1 + x2 v2 with x1 = k b2 / det, x2 = -k b1 / det: the routine approximates |x_i| from above zero and
    # the signs s_i of x_i go into the constants it multiplies by
    s1 = 1 if b2 * det >= 0 else -1
    s2 = 1 if -b1 * det >= 0 else -1
    g1 = ((abs(b2) << 256) + r // 2) // r
    g2 = ((abs(b1) << 256) + r // 2) // r
    # k1 = k - (s1 c1) a1 - (s2 c2) a2, k2 = -(s1 c1) b1 - (s2 c2) b2, the constants mod 2^256 (two's complement)
    consts = {"LAMBDA": lam, "BETA": c.base.to_mont(beta), "G1": g1, "G2": g2,
              "NA1": (-s1 * a1) & M256, "NA2": (-s2 * a2) & M256, "NB1": (-s1 * b1) & M256, "NB2": (-s2 * b2) & M256}
    vec = ((a1, b1), (a2, b2))
    return consts, vec, (lam, beta)


def split(k, consts):
    """the routine of h2_group_fft.hpp in Python integers: (|k1|, |k2|, neg1, neg2)"""
    c1, c2 = (k * consts["G1"]) >> 256, (k * consts["G2"]) >> 256
    k1 = (k + c1 * consts["NA1"] + c2 * consts["NA2"]) & M256
    k2 = (c1 * consts["NB1"] + c2 * consts["NB2"]) & M256
    n1, n2 = k1 >> 255, k2 >> 255
    return ((-k1) & M256 if n1 else k1), ((-k2) & M256 if n2 else k2), n1, n2


def bound(vec, r):
    """bits that hold |k1| and |k2| for every k < 2^256: (k, 0) = x1 v1 + x2 v2 exactly with real x_i; the routine takes
    c_i = floor(k g_i / 2^256) with g_i = x_i 2^256 / k rounded, so 0 <= x_i - c_i < 1 + k / 2^257 <= 1.5, and the
    remainder (k1, k2) = (x1 - c1) v1 + (x2 - c2) v2 has |coordinate| < 1.5 (|v1| + |v2|) coordinate-wise"""
    worst = 0
    for j in (0, 1):
        worst = max(worst, 3 * (abs(vec[0][j]) + abs(vec[1][j])) // 2 + 1)
    return worst.bit_length()


def cpp_inc(check_pairing=True):
    def fn(name, v):
        assert 0 <= v <= M256
        return ("  static H2_HD constexpr uint32_t %s(int i) { const uint32_t t[8] = {%s}; return t[i]; }"
                % (name, ", ".join("0x%08xu" % ((v >> (32 * i)) & 0xFFFFFFFF) for i in range(8))))
    out = ["// GENERATED by tools/glv_constants.py -- do not edit.",
           "// GLV split of a scalar along the cube-root endomorphism (x, y) -> (beta x, y) = [lambda](x, y).",
           "// 8 x u32 little-endian limbs.  LAMBDA: canonical integer; BETA: Montgomery R = 2^256 in the base field;",
           "// G1, G2: c_i = floor(k G_i / 2^256); NA*, NB*: the negated basis coordinates mod 2^256 (two's complement):",
           "// k1 = k + c1 NA1 + c2 NA2, k2 = c1 NB1 + c2 NB2 (mod 2^256, read as signed).  BITS: |k1|, |k2| < 2^BITS.",
           "// Keyed by the curve's SCALAR field (one curve each); BETA lives in that curve's base field.",
           "template <class FS> struct Glv;"]
    bits = 0
    for name in CURVE_ORDER:
        consts, vec, _ = derive(name, check_pairing)
        b = bound(vec, R.CURVES[name].scalar.p)
        bits = max(bits, b)
        out.append("template <> struct Glv<%s> {   // %s" % (R.CURVES[name].scalar.name.upper(), name))
        for key in ("LAMBDA", "BETA", "G1", "G2", "NA1", "NA2", "NB1", "NB2"):
            out.append(fn(key, consts[key]))
        out.append("  static constexpr int BITS = %d;" % b)
        out.append("};")
    out.append("constexpr int GLV_BITS = %d;   // the largest of the three: the joint double-and-add's loop length" % bits)
    return "\n".join(out) + "\n"


def main():
    import random
    rng = random.Random(0x474C56)
    for name in CURVE_ORDER:
        consts, vec, (lam, beta) = derive(name)
        r = R.CURVES[name].scalar.p
        b = bound(vec, r)
        worst = 0
        for k in [0, 1, 2, r - 1, lam, lam * lam % r, r - lam, M256] + [rng.randrange(r) for _ in range(20000)]:
            m1, m2, n1, n2 = split(k, consts)
            assert ((-m1 if n1 else m1) + (-m2 if n2 else m2) * lam - k) % r == 0
            assert m1 < (1 << b) and m2 < (1 << b), (name, hex(k))
            worst = max(worst, m1.bit_length(), m2.bit_length())
        print("%s: basis %d / %d / %d / %d bits, proven bound %d bits, largest seen %d bits" % (
            name, *(abs(x).bit_length() for v in vec for x in v), b, worst))
    with open(os.path.join(ROOT, "halo2_prover_amd", "csrc", "h2_glv_constants.inc"), "w") as f:
        f.write(cpp_inc())
    print("constants written")


if __name__ == "__main__":
    main()
