// h2_sqrt.hpp -- square roots in the base field of the three curves, one lane per element, on the 29-bit working form
// (h2_field29.hpp).  ONE __host__ __device__ function: the CPU tests run its host instantiation (h2_selftest_host, what = 10
// and 11) against big integers.
//
// BN254 (q = 3 mod 4): the single power a^((q + 1) / 4), as g1_decompress always took it.
//
// Pallas and Vesta (q - 1 = 2^32 t, t odd): w = a^((t - 1) / 2) from a compile-time exponent, v = a w, b = v w = a^t in
// mu_(2^32).  With g the fixed generator of mu_(2^32) (g = z^t, z the smallest non-residue) and b = g^e, a is a square iff
// e is even, and then sqrt(a) = v g^(-e / 2).  e is taken four bits at a time (Pohlig-Hellman): with x_i = b^(2^(28 - 4 i))
// and the digits e_0 .. e_(i-1) known,
//     y = x_i prod_{j < i} g^(-e_j 2^(28 - 4 (i - j))) = h^(e_i),   h = g^(2^28) of order 16,
// and the four bits of e_i come off one at a time: y^8 = (-1)^(bit 0), y <- y h^(-bit 0), y^4 = (-1)^(bit 1), ...  A power
// that can only be +1 or -1 is told apart by its lowest limb (q = 1 mod 2^29: a lazily reduced value differs from the
// canonical one by a small multiple of q, which moves that limb by as much; tools/pasta_sqrt_constants.py asserts the
// distance).  Every factor g^(...) comes from a table indexed by the digit or the bit (PastaSqrt<FP>::T, generated, 256
// elements in the working form): the data enters through table indices and selects only.  No trip count and no branch
// depends on the element -- a wave mixes residues, non-residues and elements of every order 2^j at no cost.  An odd e
// is not tested for: the halved digit gives v g^(-(e - 1) / 2), whose square is a g, and the one check every caller makes,
// root^2 == a, refuses it like any other non-square.
//
// Products per element, exact (tools/pasta_sqrt_constants.py prints them):
//     a^2, a^3 and the power a^((t - 1) / 2), two exponent bits at a time   221 squarings + 35 products (Vesta's field: 33)
//     v and b                                                                            2 products
//     x_0 .. x_7                                                             28 squarings
//     eight windows: 6 squarings + 3 products each, 0 + 1 + ... + 7 digit corrections
//                                                                            48 squarings + 52 products
//     the root v prod_j F_j[e_j]                                                          8 products
//     root^2 == a                                                             1 squaring
// 395 in all (393), 136 of them for the discrete logarithm and the root, against 496 squarings + 32 products for the
// bit-by-bit constant-time Tonelli-Shanks (c (c - 1) / 2 squarings for c = 32); BN254's single power is 253 squarings and
// at most 127 products.
#pragma once
#include "h2_curve.hpp"
#include "h2_field29.hpp"

namespace h2 {

#include "h2_pasta_sqrt_constants.inc"

template <class FP>
constexpr bool sqrt_by_one_power() { return (FP::P(0) & 3u) == 3u; }

template <class FP>
H2_HD Fe29<FP> pasta_sqrt_entry(uint32_t i) {
  Fe29<FP> r;
#pragma unroll
  for (int l = 0; l < 9; l++) r.v[l] = PastaSqrt<FP>::T(9 * i + l);
  return r;
}

// the discrete logarithm of b = x[7] in mu_(2^32) to the base g, four bits per window
template <class FP>
struct PastaSqrtWindows {
  using W = Fe29<FP>;
  W x[8];
  uint32_t dig[8];
  // s = 1 or -1 (for a = 0: 0, which reads as "not one"; the digits are then garbage and the root, v times them, is 0)
  static H2_HD uint32_t not_one(const W& s) {
    return (((uint32_t)(s.v[0] - PastaSqrt<FP>::ONE0 + 4)) & L29_MASK) < 8u ? 0u : 1u;
  }
  template <int I>
  H2_HD void powers() {
    if constexpr (I >= 0) {
      x[I] = fe29_sqr(fe29_sqr(fe29_sqr(fe29_sqr(x[I + 1]))));
      powers<I - 1>();
    }
  }
  template <int I, int J>
  H2_HD W corrected(const W& yv) const {
    if constexpr (J < I) return corrected<I, J + 1>(fe29_mul(yv, pasta_sqrt_entry<FP>(16u * (uint32_t)(I - J) + dig[J])));
    else return yv;
  }
  template <int I>
  H2_HD void window() {
    if constexpr (I < 8) {
      W yv = corrected<I, 0>(x[I]);
      const uint32_t d0 = not_one(fe29_sqr(fe29_sqr(fe29_sqr(yv))));
      yv = fe29_mul(yv, pasta_sqrt_entry<FP>(d0));
      const uint32_t d1 = not_one(fe29_sqr(fe29_sqr(yv)));
      yv = fe29_mul(yv, pasta_sqrt_entry<FP>(2u * d1));
      const uint32_t d2 = not_one(fe29_sqr(yv));
      yv = fe29_mul(yv, pasta_sqrt_entry<FP>(4u * d2));
      dig[I] = d0 | (d1 << 1) | (d2 << 2) | (not_one(yv) << 3);
      window<I + 1>();
    }
  }
};

// a: normalised limbs, |a| < 3p/2 (canonical, or a product's result) -> y with y^2 = a if a is a square, anything else
// (|y| < 3p/2, normalised) if it is not
template <class FP>
H2_HD Fe29<FP> fe29_sqrt_candidate(const Fe29<FP>& a) {
  using W = Fe29<FP>;
  const W a2 = fe29_sqr(a), a3 = fe29_mul(a2, a);
  if constexpr (sqrt_by_one_power<FP>()) {
    static_assert((FP::P(7) >> 30) == 0 && ((FP::P(7) >> 29) & 1u) == 1u, "q has 254 bits: (q + 1) / 4 has 252");
    // y = a^((q + 1) / 4), two exponent bits at a time from the top; every operand is below 3p/2 in magnitude
    uint32_t e[8];
#pragma unroll
    for (int w = 0; w < 8; w++) {                              // (q + 1) >> 2: the + 1 stays inside the lowest word (q = ...11)
      const uint64_t lo = (uint64_t)FP::P(w) + (w == 0 ? 1u : 0u), hi = w + 1 < 8 ? FP::P(w + 1) : 0;
      e[w] = (uint32_t)((lo | (hi << 32)) >> 2);
    }
    W y = fe29_from_api(Fe<FP>::one());
    for (int i = 250; i >= 0; i -= 2) {
      y = fe29_sqr(fe29_sqr(y));
      const uint32_t d = (e[i >> 5] >> (i & 31)) & 3u;
      if (d == 1) y = fe29_mul(y, a);
      else if (d == 2) y = fe29_mul(y, a2);
      else if (d == 3) y = fe29_mul(y, a3);
    }
    return y;
  } else {
    static_assert(FP::TWO_ADICITY == 32 && FP::P(0) == 1u && (FP::P(7) >> 29) == 2u,
                  "q = 1 mod 2^32 with 255 bits: (t - 1) / 2 = q >> 33 has 222 bits, and q = 1 mod 2^29 for the +-1 test");
    // w = a^(q >> 33): the top digit (bits 221, 220 = binary 10) seeds the power
    uint32_t e[8];
#pragma unroll
    for (int w = 0; w < 8; w++) {
      const uint32_t lo = w + 1 < 8 ? FP::P(w + 1) : 0u, hi = w + 2 < 8 ? FP::P(w + 2) : 0u;
      e[w] = (lo >> 1) | (hi << 31);
    }
    W y = a2;
    for (int i = 218; i >= 0; i -= 2) {
      y = fe29_sqr(fe29_sqr(y));
      const uint32_t d = (e[i >> 5] >> (i & 31)) & 3u;
      if (d == 1) y = fe29_mul(y, a);
      else if (d == 2) y = fe29_mul(y, a2);
      else if (d == 3) y = fe29_mul(y, a3);
    }
    const W v = fe29_mul(y, a), b = fe29_mul(v, y);           // a^((t + 1) / 2), a^t
    // x[i] = b^(2^(28 - 4 i)); the windows are instantiated one by one (PastaSqrtWindows below): every index into x and
    // dig is a constant from the front end on, so both are registers whatever the unroller decides
    PastaSqrtWindows<FP> ws;
    ws.x[7] = b;
    ws.template powers<6>();
    ws.template window<0>();
    const uint32_t* dig = ws.dig;
    W r = v;
#pragma unroll
    for (int j = 0; j < 8; j++) r = fe29_mul(r, pasta_sqrt_entry<FP>(16u * (uint32_t)(8 + j) + dig[j]));
    return r;
  }
}

// the square root with the wanted parity of its canonical integer, in the API form, and whether a is a square at all (the
// caller drops `out` if not).  Every lane runs every product
template <class FP>
H2_HD bool fe29_sqrt_parity(const Fe29<FP>& a, uint32_t parity, Fe<FP>& out) {
  const Fe29<FP> y = fe29_sqrt_candidate(a);
  // y^2 == a ?  |y^2 - a| < 3p: within fe29_to_api's reach
  const bool square = fe29_to_api(fe29_sub(fe29_sqr(y), a)).is_zero();
  // the parity of y as an integer: y R' / R' through a product with the plain integer 1
  Fe29<FP> plain_one = Fe29<FP>::zero();
  plain_one.v[0] = 1;
  const Fe<FP> y_int = fe29_canonical_pack(fe29_mul(y, plain_one));
  Fe<FP> ym = fe29_to_api(y);
  if ((y_int.v[0] & 1u) != parity) ym = fe_neg(ym);
  out = ym;
  return square;
}

constexpr uint8_t SQRT_OK = 0, SQRT_NOT_CANONICAL = 1, SQRT_NOT_A_SQUARE = 3;

// x < q ?  (the borrow of x - q)
template <class FP>
H2_HD bool fe_below_modulus(const Fe<FP>& x) {
  uint64_t br = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const uint64_t d = (uint64_t)x.v[i] - FP::P(i) - br;
    br = (d >> 63) & 1;
  }
  return br != 0;
}

// one element in the API form (Montgomery limbs) -> status, and for status 0 its even square root in the API form; zero
// for every other status.  A refused lane still runs the chain (on zero) and drops the result.
template <class FP>
H2_HD uint8_t base_sqrt(const Fe<FP>& in, Fe<FP>& out) {
  const bool canonical = fe_below_modulus(in);
  Fe<FP> root = Fe<FP>::zero();
  const bool square = fe29_sqrt_parity(fe29_from_api(canonical ? in : Fe<FP>::zero()), 0u, root);
  const uint8_t status = !canonical ? SQRT_NOT_CANONICAL : !square ? SQRT_NOT_A_SQUARE : SQRT_OK;
  out = status == SQRT_OK ? root : Fe<FP>::zero();
  return status;
}

// one lane per element; d_out may be d_in: a lane reads its element before it writes it
template <class FP>
__global__ void __launch_bounds__(64)
base_sqrt_kernel(const U128* in, U128* out, uint8_t* __restrict__ status, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Fe<FP> r;
  const uint8_t st = base_sqrt<FP>(fe_load<FP>(in + 2 * (size_t)i), r);
  fe_store<FP>(out + 2 * (size_t)i, r);
  status[i] = st;
}

}  // namespace h2
