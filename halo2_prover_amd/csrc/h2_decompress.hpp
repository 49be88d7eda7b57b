// h2_decompress.hpp -- batched decompression of G1 points in the transcript's wire form (Blake2bRead::read_point,
// SURVEY.md App. A.5): 32 bytes = x little-endian, bit 6 of the last byte the parity of y, bit 7 the identity flag.
//
// The batch verifier (h2_verify_proofs, h2_prover.hip) knows where the points of a proof sit before it has hashed a
// byte of it, so the one square root per point -- most of what the host spends replaying a transcript: 0.06 ms per proof
// are left without it -- is taken for the whole batch in one launch, one lane per point.  Only for base fields with q = 3 mod 4, where
// sqrt(a) = a^((q + 1) / 4): BN254.  The Pasta fields (2-adicity 32) would need Tonelli-Shanks and have no entry in
// their CurveOps.
//
// The arithmetic is ONE __host__ __device__ function on the 29-bit working form (h2_field29.hpp); the CPU tests run its
// host instantiation (h2_selftest_host, what = 8) against big integers.  The exponent is a compile-time constant, so
// every lane takes the same branches: 252 squarings and at most 126 products by a, a^2 or a^3, then one squaring for the
// residue check, one product for the parity and one to leave the working form.
#pragma once
#include "h2_curve.hpp"
#include "h2_field29.hpp"

namespace h2 {

constexpr uint8_t DECOMPRESS_OK = 0, DECOMPRESS_NOT_CANONICAL = 1, DECOMPRESS_IDENTITY = 2, DECOMPRESS_NOT_ON_CURVE = 3;

// one compressed point (eight little-endian words) -> status, and for status 0 the affine point in the API form
// (Montgomery limbs, R = 2^256); x and y are zero for every other status.  The decision and the coordinates are those of
// Transcript::read_point (h2_prover.hip) for every input.
template <class CV>
H2_HD uint8_t g1_decompress(const uint32_t in[8], Fe<typename CV::Base>& out_x, Fe<typename CV::Base>& out_y) {
  using FP = typename CV::Base;
  static_assert((FP::P(0) & 3u) == 3u, "square roots by one power need q = 3 mod 4");
  static_assert((FP::P(7) >> 30) == 0 && ((FP::P(7) >> 29) & 1u) == 1u, "q has 254 bits: (q + 1) / 4 has 252");
  const uint32_t sign = (in[7] >> 30) & 1u, inf = in[7] >> 31;
  Fe<FP> xi;
#pragma unroll
  for (int i = 0; i < 8; i++) xi.v[i] = in[i];
  xi.v[7] &= 0x3FFFFFFFu;
  // x < q ?  (the borrow of x - q)
  uint64_t br = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const uint64_t d = (uint64_t)xi.v[i] - FP::P(i) - br;
    br = (d >> 63) & 1;
  }
  const bool canonical = br != 0;
  const bool identity = inf != 0 || (xi.is_zero() && sign == 0);
  // a lane whose x is refused still runs the chain below (on x as it is: nothing in it can trap) and drops the result
  const Fe<FP> xm = fe_to_mont(xi);                          // the API form of x
  Fe<FP> bm;
#pragma unroll
  for (int i = 0; i < 8; i++) bm.v[i] = CV::B(i);
  const Fe29<FP> x = fe29_from_api(xm), one = fe29_from_api(Fe<FP>::one());
  const Fe29<FP> x3 = fe29_mul(fe29_sqr(x), x);             // in (-3p/2, p/2]
  // a = x^3 + b: the curve constant is canonical, so |a| < 3p/2; limbs normalised for the squarings
  const Fe29<FP> a = fe29_norm(fe29_add(x3, fe29_from_api(bm)));
  const Fe29<FP> a2 = fe29_sqr(a), a3 = fe29_mul(a2, a);
  // y = a^((q + 1) / 4), two exponent bits at a time from the top; every operand is below 3p/2 in magnitude
  uint32_t e[8];
#pragma unroll
  for (int w = 0; w < 8; w++) {                              // (q + 1) >> 2: the + 1 stays inside the lowest word (q = ...11)
    const uint64_t lo = (uint64_t)FP::P(w) + (w == 0 ? 1u : 0u), hi = w + 1 < 8 ? FP::P(w + 1) : 0;
    e[w] = (uint32_t)((lo | (hi << 32)) >> 2);
  }
  Fe29<FP> y = one;
  for (int i = 250; i >= 0; i -= 2) {
    y = fe29_sqr(fe29_sqr(y));
    const uint32_t d = (e[i >> 5] >> (i & 31)) & 3u;
    if (d == 1) y = fe29_mul(y, a);
    else if (d == 2) y = fe29_mul(y, a2);
    else if (d == 3) y = fe29_mul(y, a3);
  }
  // y^2 == a ?  |y^2 - a| < 3p: within fe29_to_api's reach
  const bool on_curve = fe29_to_api(fe29_sub(fe29_sqr(y), a)).is_zero();
  // the parity of y as an integer: y R' / R' through a product with the plain integer 1
  Fe29<FP> plain_one = Fe29<FP>::zero();
  plain_one.v[0] = 1;
  const Fe<FP> y_int = fe29_canonical_pack(fe29_mul(y, plain_one));
  Fe<FP> ym = fe29_to_api(y);
  if ((y_int.v[0] & 1u) != sign) ym = fe_neg(ym);
  const uint8_t status = !canonical ? DECOMPRESS_NOT_CANONICAL : identity ? DECOMPRESS_IDENTITY
                         : !on_curve ? DECOMPRESS_NOT_ON_CURVE : DECOMPRESS_OK;
  out_x = status == DECOMPRESS_OK ? xm : Fe<FP>::zero();
  out_y = status == DECOMPRESS_OK ? ym : Fe<FP>::zero();
  return status;
}

// one lane per point; status bytes go out as ordinary byte stores
template <class CV>
__global__ void __launch_bounds__(64)
points_decompress_kernel(const uint32_t* __restrict__ in /* n x 8 words */, U128* __restrict__ out /* n x 64 bytes */,
                         uint8_t* __restrict__ status, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  using FB = typename CV::Base;
  const U128 lo = reinterpret_cast<const U128*>(in)[2 * (size_t)i], hi = reinterpret_cast<const U128*>(in)[2 * (size_t)i + 1];
  const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
  Fe<FB> x, y;
  const uint8_t st = g1_decompress<CV>(w, x, y);
  fe_store<FB>(out + 4 * (size_t)i, x);
  fe_store<FB>(out + 4 * (size_t)i + 2, y);
  status[i] = st;
}

}  // namespace h2
