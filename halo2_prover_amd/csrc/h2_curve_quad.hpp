// h2_curve_quad.hpp -- XYZZ point arithmetic with FOUR LANES PER POINT (gfx950 DPP quad_perm), on the MSM's working
// field representation (h2_field29.hpp / h2_curve29.hpp).
//
// The tail of the MSM (summing a bucket's pieces, the bucket weights, the final tree) works on few points with long
// dependency chains: about one wave per SIMD, every addition waiting for the previous one.  A full XYZZ addition is
// 14 field multiplications executed one after the other by a lane, but its dependency DEPTH is 4:
//     level 1   u1 = x1 zz2      u2 = x2 zz1      s1 = y1 zzz2     s2 = y2 zzz1
//     level 2   pp = p^2         rr = r^2         zz12 = zz1 zz2   zzz12 = zzz1 zzz2        (p = u2-u1, r = s2-s1)
//     level 3   ppp = p pp       q = u1 pp        zz3 = zz12 pp
//     level 4   r (q - x3)       s1 ppp           zzz3 = zzz12 ppp                          (x3 = rr - ppp - 2q)
// Here the four lanes of a quad hold the same two points; at each level every lane selects the operands of ITS
// product (mask arithmetic on the lane's role), all four execute the same multiplication, and the results are passed
// around with v_mov_b32 quad_perm moves (one VALU instruction per word, no LDS; which lane computes what, and what is
// broadcast, is laid out under ROUTED OPERANDS below).  A lone wave is issue-bound
// (~4.5 cycles per VALU instruction whatever the dependencies), so what counts is instructions per operation: about a
// third of the one-lane form.  History of the measurements (Poseidon k = 16 bench, per MSM phase, 32-bit limbs):
// weights 192 -> 131 us and tree 190 -> 131 us with the first version, 86 / 96 us once the operand select was
// written as mask arithmetic (as `q == 0 ? a0 : ...` it compiled to exec-mask branches and the points lived in
// scratch), fix-up 188 -> 117 us; on the 29-bit working form 64 / 65 / 74 us.
//
// Contract: a and b are REPLICATED across the quad (all four lanes hold identical values) and so is the result.
// All four lanes of a quad must be active and take the same branches (they do: the data is replicated).
#pragma once
#include "h2_curve.hpp"
#include "h2_curve29.hpp"

namespace h2 {

template <int R>
__device__ __forceinline__ uint32_t quad_bcast_u32(uint32_t v) {
  // dpp_ctrl quad_perm:[R,R,R,R]; all rows / banks enabled; bound_ctrl irrelevant (source lane is in the quad)
  uint32_t r = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, R * 0x55, 0xf, 0xf, true);
  asm volatile("" : "+v"(r));   // keep it a plain v_mov_b32_dpp (see the note below)
  return r;
}
// the operand of lane role q among four candidates, as mask arithmetic: as `q == 0 ? a0 : ...` the compiler turned
// every word into exec-mask branches.  (m & a) | (~m & b) is ONE v_bitop3_b32 (truth table 0xCA), asked for by name:
// from the C expression the compiler built v_and_b32 + v_and_or_b32 against a hoisted ~m, two instructions per word.
__device__ __forceinline__ uint32_t quad_bfi(uint32_t m, uint32_t a, uint32_t b) {
  return (uint32_t)__builtin_amdgcn_bitop3_b32((int)m, (int)a, (int)b, 0xCA);
}

// The broadcast words feed ordinary VALU code, and with ROCm 7.2 the compiler's folding of v_mov_b32_dpp into the
// consuming instruction produced wrong results for every input (tests/test_gpu_parity.py::
// test_device_group_law_on_the_working_form failed on ops 0 and 1 while the one-lane forms passed): quad_bcast_u32
// pins its result with an empty asm statement.
template <int R, class FP>
__device__ __forceinline__ Fe29<FP> quad_bcast(const Fe29<FP>& a) {
  Fe29<FP> r;
#pragma unroll
  for (int i = 0; i < 9; i++) r.v[i] = (int32_t)quad_bcast_u32<R>((uint32_t)a.v[i]);
  return r;
}
template <class FP>
__device__ __forceinline__ Fe29<FP> quad_select(uint32_t q, const Fe29<FP>& a0, const Fe29<FP>& a1, const Fe29<FP>& a2,
                                                const Fe29<FP>& a3) {
  Fe29<FP> r;
  const uint32_t m1 = 0u - (q & 1u), m2 = 0u - ((q >> 1) & 1u);
#pragma unroll
  for (int i = 0; i < 9; i++)
    r.v[i] = (int32_t)quad_bfi(m2, quad_bfi(m1, (uint32_t)a3.v[i], (uint32_t)a2.v[i]),
                               quad_bfi(m1, (uint32_t)a1.v[i], (uint32_t)a0.v[i]));
  return r;
}

// ROUTED OPERANDS.  The first version broadcast every level's four products to all four lanes (36 moves) and let each
// lane select its next operands again (two 4-way selects, three 2-way selects a word each).  Most products have one
// consumer, so the lane roles are now laid out level by level such that a product is consumed on the lane that
// computed it, or reaches its consumer with one quad_perm move per word; only what every lane needs is broadcast (pp,
// the terms of x3, the output coordinates).  The differences p and r come from ONE swapped move:
// d = m1 - quad_perm[1,0,3,2](m1) is (-p, p, -r, r) on lanes 0..3, and (-p)(-p) is the same integer product as p p,
// so the squares are taken where the difference already is.  A lane without a product at some level multiplies
// operands that are within the limb bounds and its result is never read.  Every product that IS read has the integer
// operands of the first version, so the result limbs are unchanged (tests/test_gpu_xyzz29_ranges.py holds them
// against pyref's model of that version).  Measured, lone wave: addition 2.84 -> 2.50 us, doubling 2.30 -> 2.09 us
// (profiles/quad_ops_parent_vs_branch.txt); four products are 2.0 us of the addition.
template <int S0, int S1, int S2, int S3>
__device__ __forceinline__ uint32_t quad_perm_u32(uint32_t v) {
  // lane i of each quad reads lane S_i
  uint32_t r = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, S0 | (S1 << 2) | (S2 << 4) | (S3 << 6), 0xf, 0xf, true);
  asm volatile("" : "+v"(r));   // as in quad_bcast_u32
  return r;
}
template <int S0, int S1, int S2, int S3, class FP>
__device__ __forceinline__ Fe29<FP> quad_perm(const Fe29<FP>& a) {
  Fe29<FP> r;
#pragma unroll
  for (int i = 0; i < 9; i++) r.v[i] = (int32_t)quad_perm_u32<S0, S1, S2, S3>((uint32_t)a.v[i]);
  return r;
}
// m ? a : b, word by word (m is all ones or all zeros)
template <class FP>
__device__ __forceinline__ Fe29<FP> quad_pick(uint32_t m, const Fe29<FP>& a, const Fe29<FP>& b) {
  Fe29<FP> r;
#pragma unroll
  for (int i = 0; i < 9; i++) r.v[i] = (int32_t)quad_bfi(m, (uint32_t)a.v[i], (uint32_t)b.v[i]);
  return r;
}
// the one-limb filter of fe29_is_zero_mod_p: false means a is certainly not 0 mod p
template <class FP>
__device__ __forceinline__ bool fe29_maybe_zero_mod_p(const Fe29<FP>& a) {
  constexpr uint32_t pinv = (0u - (FP::INV & L29_MASK)) & L29_MASK;
  const uint32_t j = ((uint32_t)a.v[0] * pinv) & L29_MASK;
  return !(j > 16u && j < (1u << 29) - 16u);
}

template <class CV>
__device__ __forceinline__ Xyzz29<CV> xyzz29_double_quad(const Xyzz29<CV>& p) {
  using F = Fe29<typename CV::Base>;
  if (p.is_identity() || fe29_is_zero_mod_p(p.y)) return Xyzz29<CV>::identity();
  const uint32_t q = threadIdx.x & 3;
  const uint32_t odd = 0u - (q & 1u), hi = 0u - (q >> 1), is0 = ~(odd | hi), is2 = hi & ~odd;
  const F u = fe29_norm(fe29_add(p.y, p.y));
  // level 1: v = u^2 (lane 0), xx = x^2 (lanes 1..3, where m = 3 xx is formed)
  const F o1 = quad_pick(is0, u, p.x);
  const F m1 = fe29_mul(o1, o1);
  const F v = quad_bcast<0>(m1);
  const F m = fe29_norm(fe29_add(fe29_add(m1, m1), m1));
  // level 2: w = u v, s = x v, mm = m^2, zz3 = v zz
  const F m2 = fe29_mul(quad_pick(hi, quad_pick(odd, p.zz, m), o1), quad_pick(is2, m, v));
  const F w = quad_bcast<0>(m2), s = quad_bcast<1>(m2), mm = quad_bcast<2>(m2), zz3 = quad_bcast<3>(m2);
  const F x3 = fe29_norm(fe29_sub(fe29_sub(mm, s), s));
  // level 3: w y, zzz3 = w zzz, m (s - x3) on lane 2, which holds m
  const F m3 = fe29_mul(quad_pick(is2, m, w), quad_pick(is2, fe29_sub(s, x3), quad_pick(odd, p.zzz, p.y)));
  const F y3 = fe29_norm(fe29_sub(quad_bcast<2>(m3), quad_bcast<0>(m3)));
  return Xyzz29<CV>{x3, y3, zz3, quad_bcast<1>(m3)};
}

template <class CV>
__device__ __forceinline__ Xyzz29<CV> xyzz29_add_quad(const Xyzz29<CV>& a, const Xyzz29<CV>& b) {
  using F = Fe29<typename CV::Base>;
  if (a.is_identity()) return b;
  if (b.is_identity()) return a;
  const uint32_t q = threadIdx.x & 3;
  const uint32_t odd = 0u - (q & 1u), hi = 0u - (q >> 1);
  // level 1: u1 = x1 zz2, u2 = x2 zz1, s1 = y1 zzz2, s2 = y2 zzz1 on lanes 0..3
  const F m1 = fe29_mul(quad_select(q, a.x, b.x, a.y, b.y), quad_select(q, b.zz, a.zz, b.zzz, a.zzz));
  // d = (-p, p, -r, r) with p = u2 - u1, r = s2 - s1
  const F d = fe29_sub(m1, quad_perm<1, 0, 3, 2>(m1));
  if (quad_bcast_u32<1>(fe29_maybe_zero_mod_p(d) ? 1u : 0u)) {           // the filter on p, the same on all four lanes
    if (fe29_is_zero_mod_p(quad_bcast<1>(d))) {
      if (fe29_is_zero_mod_p(quad_bcast<3>(d))) return xyzz29_double_quad(a);
      return Xyzz29<CV>::identity();
    }
  }
  // level 2: pp = (-p)^2, zzz12 = zzz1 zzz2, rr = (-r)^2, zz12 = zz1 zz2
  const F m2 = fe29_mul(quad_pick(odd, quad_pick(hi, a.zz, a.zzz), d), quad_pick(odd, quad_pick(hi, b.zz, b.zzz), d));
  const F pp = quad_bcast<0>(m2);
  // level 3: qq = u1 pp, ppp = p pp, -, zz3 = zz12 pp: each lane's left operand is its own
  const F m3 = fe29_mul(quad_pick(hi, m2, quad_pick(odd, d, m1)), pp);
  const F qq = quad_bcast<0>(m3), ppp = quad_bcast<1>(m3), rr = quad_bcast<2>(m2);
  const F x3 = fe29_norm(fe29_sub(fe29_sub(fe29_sub(rr, ppp), qq), qq));
  // level 4: -, zzz3 = zzz12 ppp, s1 ppp, r (qq - x3)
  const F m4 = fe29_mul(quad_pick(odd, quad_pick(hi, d, m2), m1), quad_pick(odd & hi, fe29_sub(qq, x3), ppp));
  const F y3 = fe29_norm(fe29_sub(quad_bcast<3>(m4), quad_bcast<2>(m4)));
  return Xyzz29<CV>{x3, y3, quad_bcast<3>(m3), quad_bcast<1>(m4)};
}

}  // namespace h2
