// h2_decompress.hpp -- batched decompression of G1 points in the transcript's wire form (Blake2bRead::read_point,
// SURVEY.md App. A.5): 32 bytes = x little-endian, bit 6 of the last byte the parity of y, bit 7 the identity flag.
//
// The batch verifier (h2_verify_proofs, h2_prover.hip) knows where the points of a proof sit before it has hashed a
// byte of it, so the one square root per point -- most of what the host spends replaying a transcript: 0.06 ms per proof
// are left without it -- is taken for the whole batch in one launch, one lane per point.  That wire
// form is BN254's, where q = 3 mod 4 and sqrt(a) = a^((q + 1) / 4); h2_points_decompress_device and h2_verify_proofs stay
// BN254's (the Pasta curves have no points_decompress in their CurveOps).  The Pasta wire form (transcript.py: bit 255 the
// parity of y, 32 zero bytes the identity, no identity flag) is pasta_decompress below, behind
// h2_pasta_points_decompress_device: the inner product argument's batch verifier (ipa.verify_proofs) is its caller.
//
// The arithmetic is ONE __host__ __device__ function per wire form on the 29-bit working form (h2_field29.hpp); the CPU
// tests run the host instantiations (h2_selftest_host, what = 8 and 10) against big integers.  The square root is
// h2_sqrt.hpp's: for BN254 a compile-time exponent, 252 squarings and at most 126 products by a, a^2 or a^3; for the Pasta
// fields the power a^((t - 1) / 2) and a discrete logarithm in mu_(2^32) by table.  Every lane takes the same branches.
// Then one squaring for the residue check, one product for the parity and one to leave the working form.
#pragma once
#include "h2_curve.hpp"
#include "h2_field29.hpp"
#include "h2_sqrt.hpp"

namespace h2 {

constexpr uint8_t DECOMPRESS_OK = 0, DECOMPRESS_NOT_CANONICAL = 1, DECOMPRESS_IDENTITY = 2, DECOMPRESS_NOT_ON_CURVE = 3;

// one compressed point (eight little-endian words) -> status, and for status 0 the affine point in the API form
// (Montgomery limbs, R = 2^256); x and y are zero for every other status.  The decision and the coordinates are those of
// Transcript::read_point (h2_prover.hip) for every input.
template <class CV>
H2_HD uint8_t g1_decompress(const uint32_t in[8], Fe<typename CV::Base>& out_x, Fe<typename CV::Base>& out_y) {
  using FP = typename CV::Base;
  static_assert(sqrt_by_one_power<FP>(), "this wire form (two flag bits) is BN254's; Pasta: pasta_decompress");
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
  const Fe29<FP> x = fe29_from_api(xm);
  const Fe29<FP> x3 = fe29_mul(fe29_sqr(x), x);             // in (-3p/2, p/2]
  // a = x^3 + b: the curve constant is canonical, so |a| < 3p/2; limbs normalised for the squarings
  const Fe29<FP> a = fe29_norm(fe29_add(x3, fe29_from_api(bm)));
  Fe<FP> ym = Fe<FP>::zero();
  const bool on_curve = fe29_sqrt_parity(a, sign, ym);      // y = a^((q + 1) / 4), y^2 == a, the parity (h2_sqrt.hpp)
  const uint8_t status = !canonical ? DECOMPRESS_NOT_CANONICAL : identity ? DECOMPRESS_IDENTITY
                         : !on_curve ? DECOMPRESS_NOT_ON_CURVE : DECOMPRESS_OK;
  out_x = status == DECOMPRESS_OK ? xm : Fe<FP>::zero();
  out_y = status == DECOMPRESS_OK ? ym : Fe<FP>::zero();
  return status;
}

// The same for the Pasta wire form: bit 255 the parity of y, no identity flag, the identity is x = 0 with parity 0.  The
// decision and the coordinates are those of transcript.decompress for every 32-byte input.
template <class CV>
H2_HD uint8_t pasta_decompress(const uint32_t in[8], Fe<typename CV::Base>& out_x, Fe<typename CV::Base>& out_y) {
  using FP = typename CV::Base;
  static_assert(!sqrt_by_one_power<FP>(), "this wire form (one flag bit) is the Pasta curves'");
  const uint32_t sign = in[7] >> 31;
  Fe<FP> xi;
#pragma unroll
  for (int i = 0; i < 8; i++) xi.v[i] = in[i];
  xi.v[7] &= 0x7FFFFFFFu;
  const bool canonical = fe_below_modulus(xi);
  const bool identity = xi.is_zero() && sign == 0;
  // a lane whose x is refused runs the chain below on zero and drops the result
  const Fe<FP> xm = fe_to_mont(canonical ? xi : Fe<FP>::zero());
  Fe<FP> bm;
#pragma unroll
  for (int i = 0; i < 8; i++) bm.v[i] = CV::B(i);
  const Fe29<FP> x = fe29_from_api(xm);
  const Fe29<FP> x3 = fe29_mul(fe29_sqr(x), x);             // in (-3p/2, p/2]
  const Fe29<FP> a = fe29_norm(fe29_add(x3, fe29_from_api(bm)));     // |a| < 3p/2, limbs normalised
  Fe<FP> ym = Fe<FP>::zero();
  const bool on_curve = fe29_sqrt_parity(a, sign, ym);
  const uint8_t status = !canonical ? DECOMPRESS_NOT_CANONICAL : identity ? DECOMPRESS_IDENTITY
                         : !on_curve ? DECOMPRESS_NOT_ON_CURVE : DECOMPRESS_OK;
  out_x = status == DECOMPRESS_OK ? xm : Fe<FP>::zero();
  out_y = status == DECOMPRESS_OK ? ym : Fe<FP>::zero();
  return status;
}

// one lane per point, each curve in its own wire form; status bytes go out as ordinary byte stores
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
  uint8_t st;
  if constexpr (sqrt_by_one_power<FB>()) st = g1_decompress<CV>(w, x, y);
  else st = pasta_decompress<CV>(w, x, y);
  fe_store<FB>(out + 4 * (size_t)i, x);
  fe_store<FB>(out + 4 * (size_t)i + 2, y);
  status[i] = st;
}

}  // namespace h2
