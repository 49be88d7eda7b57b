// h2_poseidon_quad.hpp -- the width-3 Poseidon permutation of h2_poseidon.hpp with ONE PERMUTATION OVER THE FOUR LANES OF A
// DPP QUAD.  What runs on it -- the walker that checks Merkle membership paths and the in-place update of a resident tree --
// is in h2_poseidon_merkle.hpp.  Device only.
//
// Why.  A Merkle path is a chain of `depth` dependent hashes, and one hash on one lane is a chain of dependent products:
// a full round is 3 (S-box) x 3 words + 9 (MDS) = 18 products one after the other, a partial round 12, 816 in all for
// (8, 56), 864 for (8, 60).  Nothing a lane-per-path walker does can be shorter than depth x that.  The three words of a
// round are independent up to the MDS product, and so are its three rows:
//     lane q < 3 of a quad holds state word q
//     x   = fe29_norm(s + rc[q])             poseidon_add_rc on the lane's own word
//     y   = x^5                              three dependent products (partial round: lanes 1, 2 keep x -- quad_pick)
//     s   = m[q][0] y_0 + m[q][1] y_1 + m[q][2] y_2        y_j broadcast with quad_bcast (v_mov_b32 quad_perm, no LDS);
//                                            three independent products and two additions, the sum left un-normalised
// The dependent chain of a round is 4 products deep whatever the round's kind, (r_f + r_p) x 4 = 256 or 272 for a
// permutation.  Full and partial rounds are ONE instruction stream: a partial round computes the S-box on every lane and
// drops the result on lanes 1..3.  Lane 3 idles: it carries lane 2's word and constants, its result is never read.  A
// quad spends 4 x 272 lane-products where a lane spends 864, so where the device is full the lane form does more hashes
// per second; which form a launch takes is decided by size (POSEIDON_WALK_QUAD_MAX in h2_poseidon.hpp).
//
// Bounds.  The analysis at the top of h2_poseidon.hpp carries over word for word at T = 3, because every word sees the same
// operations in the same order on the same integers: s + rc normalised once (4 units before, carries <= 3),
// fe29_sqr / fe29_sqr / fe29_mul on normalised operands, fe29_mul(y, m) with m canonical on the narrow side, three
// products summed without a carry pass, |s| < 3.1 p.  In a partial round lanes 1 and 2 pass the normalised x (|x| < c p,
// c = 4.1) exactly as the lane form does; the S-box they compute beside it is within fe29_sqr's and fe29_mul's bounds
// like any full round's and is dropped.  A broadcast moves limbs, it changes none.  The walker feeds the permutation
// fe29_from_api of a canonical element (canonical, normalised), the normalised word 0 of the previous level and the
// capacity word: the c* = 5.1 case of that analysis does not even arise (nothing is added to a word before round 0).
// An element that is NOT canonical never reaches a product: the walker stops at it with status 2.
//
// Constants.  Round constant and MDS row differ per lane, so they cannot all come through the scalar cache as in the lane
// form.  Chosen: plain vector loads from the same table in HBM (36-byte entries, lane q reads entry 3 r + q).
//   MDS row    three entries, loaded once per permutation and KEPT IN REGISTERS: 27 VGPRs.
//   rc         one entry per round: 9 VGPRs, and the load of round r + 1's is issued at the top of round r, so its
//              latency (L2 after the first quad of a launch has touched the 7 KB table) hides under four products.
//              The last round's prefetch reads the table's first MDS entry, which is there: no branch.
// LDS is not used: a copy of the table per workgroup would cost a barrier and 7 KB per launch for loads that are already
// off the critical path.  The registers of the kernels on it are listed in h2_poseidon_merkle.hpp.
#pragma once
#include "h2_curve_quad.hpp"
#include "h2_poseidon.hpp"

namespace h2 {

#if defined(__HIPCC__)
// s: the lane's word of the state (lane q < 3 of the quad: word q; lane 3: anything within word 2's bounds), normalised or
// a sum of three products -> the lane's word of the permuted state, normalised.  All four lanes of the quad are active
template <class FS, class A = Fe29Compiler>
__device__ __forceinline__ Fe29<FS> poseidon_permute_quad(Fe29<FS> s, const Fe29<FS>* __restrict__ table, uint32_t r_f, uint32_t r_p) {
  const uint32_t q = threadIdx.x & 3, w = q < 3 ? q : 2;
  const uint32_t others = 0u - (uint32_t)(q != 0);
  const uint32_t rounds = r_f + r_p, half = r_f >> 1;
  const Fe29<FS>* const row = table + 3 * (size_t)rounds + 3 * w;
  const Fe29<FS> m0 = row[0], m1 = row[1], m2 = row[2];
  const Fe29<FS>* rc = table + w;
  Fe29<FS> c = *rc;
#pragma unroll 1
  for (uint32_t r = 0; r < rounds; r++) {
    const Fe29<FS> x = fe29_norm(fe29_add(s, c));
    rc += 3;
    c = *rc;                                         // the next round's; behind the last round: an MDS entry, not used
    const uint32_t keep = r - half < r_p ? others : 0u;   // a partial round: lanes 1.. pass x
    const Fe29<FS> y = quad_pick(keep, x, poseidon_pow5<FS, A>(x));
    s = fe29_add(fe29_add(A::template mul<FS>(quad_bcast<0>(y), m0), A::template mul<FS>(quad_bcast<1>(y), m1)),
                 A::template mul<FS>(quad_bcast<2>(y), m2));
  }
  return fe29_norm(s);
}
// ConstantLength<2> of (a, b), all three replicated across the quad -> the hash, normalised, replicated
template <class FS>
__device__ __forceinline__ Fe29<FS> poseidon_hash2_quad(const Fe29<FS>& a, const Fe29<FS>& b, const Fe29<FS>& cap2,
                                                        const Fe29<FS>* __restrict__ table, uint32_t r_f, uint32_t r_p) {
  const uint32_t q = threadIdx.x & 3;
  const Fe29<FS> word = quad_pick(0u - (uint32_t)(q == 0), a, quad_pick(0u - (uint32_t)(q == 1), b, cap2));
  return quad_bcast<0>(poseidon_permute_quad<FS>(word, table, r_f, r_p));
}
#endif  // __HIPCC__

}  // namespace h2
