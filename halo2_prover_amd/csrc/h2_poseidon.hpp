// h2_poseidon.hpp -- the Poseidon permutation at WIDTH T = 3, 5 and 9 (rate T - 1 = 2, 4, 8, S-box x^5), the ConstantLength
// sponge on it and the permutation and hash kernels, over the scalar field of a curve, on the 9 x 29-bit working form
// (h2_field29.hpp).  Every kernel and device function of the family exists once, the width a template parameter (but for the
// binary Merkle walker, kept beside the general one: h2_poseidon_merkle.hpp says why); the Merkle
// trees of ConstantLength<T - 1> hashes (arity 2, 4, 8) are in h2_poseidon_merkle.hpp, the width-3 permutation over the four
// lanes of a quad in h2_poseidon_quad.hpp.
//
// Restates the reference's circuits/src/poseidon/primitives.rs:87-132 (permute: r_f / 2 full rounds, r_p partial rounds,
// r_f / 2 full rounds; a round = add the round constants, S-box, MDS product) and :204-390 (the ConstantLength<L> sponge,
// with the capacity word LAST: state (0, .., 0, L 2^64), the message absorbed `rate` words at a time, zero-padded, one
// permutation per absorb, output = word 0), which there is generic over Spec<F, T, RATE> and here over the template
// parameter T.  The judge is oracle/pyref.py, generic in t.  The constants come from h2_poseidon_host.hpp; the kernels read
// them from a table in HBM in the working form (x 2^261 mod p, canonical, nine limbs = 36 bytes each): (r_f + r_p) x T round
// constants, then the T x T MDS row-major, then -- at T = 5 and 9 -- the sparse form of the partial rounds
// (poseidon_table_elems below).  The round and row index are the same in every lane, so the table is read through the
// scalar cache (poseidon_const) and the constants stay out of the vector registers.
//
// Two lane bodies stand behind the one name poseidon_permute<FS, T, A, SPARSE>:
//   T = 3      named state words, the rounds' 30 products inlined in two loop bodies, dense partial rounds.  Its table
//              is the dense part alone: the quad form's prefetch (h2_poseidon_quad.hpp) relies on that layout.
//   T = 5, 9   register arrays that rotate, and the partial rounds in the sparse form ("Registers and code size" below).
//
// Bounds, against the invariants at the top of h2_field29.hpp.  Write rho = p / R' (R' = 2^261): rho = 2^-7 (1 + 2^-127)
// for the Pasta primes, below 2^-7 for BN254's.  fe29_mul(a, b) needs |a_i| < 2^30, |b_j| < 2^29 and returns a value in
// (a b / R' - p, a b / R'] with normalised limbs; fe29_sqr(a) needs |a_i| < 2^29 and a^2 <= 64 p^2.  Write u = 2^29 - 1 and
// call a word "of k units" when its limbs 0..7 lie in [0, k u]: a product's result and a canonical constant (round
// constants, matrix entries) are of 1 unit, fe29_add adds units.
//   norm    fe29_norm(a) is safe for a of AT MOST 4 UNITS: the carry into a limb is at most (4 u + 3) >> 29 = 3 and
//           limb + carry <= 4 u + 3 = 2^31 - 1 does not wrap; afterwards the limbs are back in [0, 2^29) (the top limb signed:
//           below 2^26 in magnitude for any value under 64 p, four of them do not wrap), which fe29_sqr and fe29_mul's narrow
//           side ask for.  A fifth unit (5 u > 2^31) would wrap.
//   row     A state word between rounds is a row of the matrix product, at most 3 units, so s + rc has at most 4 and ONE
//           carry pass per word and round (poseidon_add_rc) is safe; without it the S-box input would have limbs of up to
//           2^31, four times fe29_sqr's bound.  T = 3 is exactly the 4-unit case: the width-3 body's row (poseidon_mds_row)
//           is its three products summed and left UN-NORMALISED, 3 units, and the round constant is the fourth.  A row of
//           T >= 4 products cannot be summed that way: poseidon_wide_row adds the T products one by one and counts units at
//           compile time; whenever the running sum reaches 4 units it is passed through fe29_norm (back to 1 unit), and so is
//           a sum that would END on 4.  The carry passes therefore stand behind the 4th product, then behind every 3rd:
//               T = 3:  t0 + t1 + t2                                               no pass, the word has 3 units
//               T = 5:  norm(t0 + t1 + t2 + t3) + t4                               1 pass,  the word has 2 units
//               T = 9:  norm(norm(t0 + t1 + t2 + t3) + t4 + t5 + t6) + t7 + t8     2 passes, the word has 3 units
//           The absorbed word of a sponge goes onto a NORMALISED state (1 + 1 units; + rc: 3).
//           The T terms of a row are T separate products.  A fused row (one reduction for sum_j m_ij y_j) would put 9 T limb
//           products and 3 T m p terms of up to 2^58 each into one 64-bit column: already at T = 3, 36 2^58 exceeds 2^63, so it
//           is not used for any field.
//   value   A term mul(y, m) with m canonical lies in (-p - |y| rho, |y| rho], so |term| < (1 + c rho) p when |y| <= c p.
//           A round's input x = s + rc then has |x| < (1 + T (1 + c rho)) p: the map c -> 1 + T (1 + c rho) contracts
//           (T rho < 1) onto its fixed point (1 + T) / (1 - T rho) = 4.10 (T = 3), 6.25 (T = 5), 10.76 (T = 9).  The first
//           round of a sponge permutation sees the normalised output of the last one (|s| < T (1 + c rho) p), a message word
//           below p and a round constant below p.  With c* = fixed point + 1 every round input of every permutation
//           satisfies
//               |x| < c* p,     c* = 5.10 (T = 3),   7.25 (T = 5),   11.76 (T = 9)
//           (the sequence starts at or below c* and moves towards the fixed point below it), and a permutation's output has
//           |s| < T (1 + c* rho) p = 3.12 p, 5.29 p, 9.83 p; from the fixed point itself it is (c* - 2) p, and the next absorb
//           closes the loop.  The Merkle walkers and tails feed a permutation canonical or normalised words and the capacity
//           word, nothing is added before round 0: there the first round's c is below 2.
//   S-box   T <= 5: x^2 < 52.6 p^2 <= 64 p^2, fe29_sqr's precondition: x2 = sqr(x) in (-p, c*^2 rho p] -- |x2| < p; x4 =
//           sqr(x2) in (-p, rho p]; x5 = mul(x4, x) with |x4 x| < c* p^2: |x5| < (1 + c* rho) p = 1.04 p (T = 3), 1.06 p.
//           T = 9: x^2 < 138.3 p^2 is OUTSIDE fe29_sqr's 64 p^2.  The first squaring is therefore fe29_mul(x, x), whose
//           contract holds for any operands within the limb bounds (x is normalised: limbs below 2^29): x2 in
//           (-p, 1.09 p].  Then x2^2 < 1.2 p^2, x4 = sqr(x2) in (-p, rho p], x5 = mul(x4, x): |x5| < 1.10 p.  Cost: 36
//           limb products more than a squaring, once per S-box -- below 1 % of a permutation.
//           All three results are normalised, so every operand is within the limb bounds.
//   MDS     y is an S-box output (|y| < 1.10 p) or, in a dense partial round, the normalised x of words 1.. (|y| < c* p):
//           the "value" bound above covers both.  Every operand of every product is normalised on the wide side and canonical
//           or normalised on the narrow side, within fe29_mul's |a_i| < 2^30, |b_j| < 2^29.
//   out     the permutation ends with fe29_norm of every word (at most 3 units): fit for fe29_to_api (limbs below 2^30 in
//           magnitude, |value| < 64 p), for the LDS of the Merkle tail and as the state an absorb adds to.
//
//   sparse  (T = 5, 9)  The r_p partial rounds run in the factored form of h2_poseidon_host.hpp (factor_partial_rounds): the
//           full round in front of them takes the pre-matrix in place of the MDS (the bounds of a full round do not depend on
//           the matrix: its entries are canonical), d0 is added to the words 1.. once (s_j + d0_j: 3 + 1 units, normalised,
//           |.| < c* p), and round k is
//               x0 = norm(s_0 + a_k)            s_0: a row's sum, 3 units at most, + 1
//               z  = norm(x0^5 + b_k)           1 + 1 units; |z| < 1.10 p + p = 2.10 p
//               s_0 <- m00 z + sum_j vhat_j s_j  T products by poseidon_wide_term (the OLD s_j): 3 units at most
//               s_j <- norm(s_j + w_j z)         1 + 1 units; every operand of every product is normalised
//           2 T - 1 products.  The words 1.. are never multiplied into something new, they only GROW: by |w_j z / R'| + p <
//           1.02 p a round.  So every POSEIDON_WIDE_REDUCE_EVERY = 8 rounds, and behind the last round, they are multiplied
//           by the field's one (the table's last entry, canonical): the value drops to (-p - |s_j| rho, |s_j| rho].  Between
//           two reductions |s_j| < B p with B = c* + 8 x 1.02 = 15.4 (T = 5), 19.9 (T = 9) -- the first stretch starts
//           from the full round's c* p, the later ones from below 1.2 p.  Then a term vhat_j s_j is below (1 + B rho) p =
//           1.13 p, 1.16 p, the term m00 z below 1.02 p, and the S-box input |x0| < (1.02 + (T - 1)(1 + B rho) + 1) p =
//           6.5 p (T = 5), 11.3 p (T = 9) < c* p: the S-box bounds above hold as they stand (T = 9 squares with the general
//           product).  The top limb of 19.9 p is below 2^28.  Behind the last partial round the words 1.. are below
//           1.2 p and normalised and s_0 is a row's sum below 10.3 p: a full round's input, as after a dense round.
//           The reductions cost (T - 1) / 8 products a round on top of the 2 T - 1.
//   The device result is a field element in every form, so it equals the dense form's and pyref's exactly; the permutation
//   kernel is built in both forms at T = 5, 9 and the tests compare them.
//
// Registers and code size.  The rounds are not unrolled: one full-round body and one partial-round body, each in a loop
// that is kept as a loop (#pragma unroll 1); the two runs of full rounds are the two trips of an outer loop around them.
// At T = 3 each body names its words and inlines its products.  A width-9 state is 81 limbs and the outputs of a full round's
// S-boxes another 81: unrolling a full round over its words and rows would put 3 T + T^2 = 108 inlined products into its
// body alone (about 2 KB each).  Instead, at T = 5 and 9, the words of a full round and the rows of its MDS product are
// LOOPS kept as loops over a register array that is ROTATED by one word per trip (poseidon_wide_rotate), so that every
// index stays a compile-time constant and nothing goes to scratch: the S-box loop takes word 0 and appends its fifth power,
// the row loop computes row i from the T outputs (the row's constants at mat + i T, a scalar address) and appends it.  The
// full-round body holds 3 + T products, the sparse partial round 3 + 2 T - 1 and the T - 1 of the reduction.  The price of the
// rotation: the register allocator keeps both ends of the rotating arrays, so the kernels hold 190 - 280 VGPRs at width 5
// (two waves per SIMD; one in the hash kernel on the compiler's products) and 320 - 500 at width 9 (one wave per SIMD),
// without scratch.  profiles/poseidon_one_family_resources.txt has every kernel, DESIGN.md section 7.19 the measurements.
//
// The product form is a template parameter (h2_field29_chain.hpp's policies).  Measured on the width-3 hash kernel (tools/
// poseidon_bench.py): while a SIMD holds one wave or none -- n <= 2^16 lanes on the 256 CUs -- the
// compiler's form is 2-3 % ahead, from two waves per SIMD on the single-chain form is, by 2 % at 2^17 and 5.6 % at 2^20.
// So the hash kernel is instantiated on both and a launch of POSEIDON_CHAIN_MIN_N lanes or more takes the chain form where
// the field has one (Pallas, Vesta); the permutation kernel and the Merkle tail stay on the compiler's form.
//
// Not here: an in-place update of a wide tree, and a form with several lanes per permutation at
// T = 5, 9.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "h2_field29.hpp"
#include "h2_field29_chain.hpp"

namespace h2 {

constexpr uint32_t POSEIDON_MAX_ROUNDS = 128;       // r_f + r_p
constexpr uint32_t POSEIDON_THREADS = 256;
constexpr uint32_t POSEIDON_MAX_BLOCKS = 1u << 20;  // beyond that the lanes stride over the rest
constexpr size_t POSEIDON_CHAIN_MIN_N = (1u << 16) + 1;   // more lanes than one wave on every SIMD of the device
// The Merkle walker and update (h2_poseidon_merkle.hpp): hashes (paths of a verify call, or hashes of one update level)
// below which a width-3 launch takes the QUAD form, four lanes per permutation; from it on the lane form.  The sweep (tools/
// poseidon_merkle_bench.py, verify at depth 20, both forms in one run, best of the windows, ms; DESIGN.md section 7.18 has
// the whole table):
//     n            2^4    2^10   2^12   2^13   2^14   2^15   2^16   2^17    2^18    2^20
//     Pallas lane  6.39   5.61   5.61   5.60   5.69   5.60   5.79   10.72   21.09   83.5
//     Pallas quad  2.69   2.72   2.81   2.94   3.15   5.54   10.01  19.38   38.47   153.6
//     BN254 lane   8.68   7.66   7.67   7.63   7.68   7.62   7.84   14.48   28.26   111.6
//     BN254 quad   3.51   3.53   3.61   3.73   4.17   7.22   13.22  26.03   51.79   207.1
// Up to 2^14 paths -- 2^16 lanes, one wave per SIMD -- the quad form is its own shorter chain (0.40 - 0.55 of the lane
// form); at 2^15 it is two waves per SIMD and level with the lane form (1 - 5 % ahead); at 2^16 the lane form, then one wave
// per SIMD itself, is 1.7 x faster, and 1.8 x where both fill the device.  So: the quad form up to 2^15 hashes, the lane
// form above.  The numbers are those of profiles/poseidon_merkle_times.json.
constexpr size_t POSEIDON_WALK_QUAD_MAX = ((size_t)1 << 15) + 1;
// Merkle tail: levels of at most this many nodes are finished by one workgroup in one launch.  The sweep of tools/
// poseidon_bench.py cannot tell 32 .. 256 apart -- a level is one hash's latency either way -- and
// has 512, where a lane hashes two nodes in turn, behind: the default is the widest level with one node per lane.  The LDS
// of the tail kernel holds up to TAIL_MAX nodes
constexpr uint32_t POSEIDON_MERKLE_TAIL = 256;
constexpr uint32_t POSEIDON_MERKLE_TAIL_MAX = 512;

// The widths whose partial rounds run in the sparse form.  Measured on the permutation kernel (tools/poseidon_wide_bench.py,
// DESIGN.md section 7.19); at T = 5, 9 the permutation kernel alone is also built in the other form, for that measurement
// and the tests.  Width 3 has the dense form only
template <int T>
constexpr bool POSEIDON_SPARSE = T != 3;
// partial rounds between two value reductions of the words 1.. in the sparse form (a power of two)
constexpr uint32_t POSEIDON_WIDE_REDUCE_EVERY = 8;

// The table of (T, r_f, r_p), R = r_f + r_p rounds, entries of 36 bytes:
//   dense part    R T round constants, the T x T MDS row-major                     (h2_poseidon_wide_constants' elements)
//   sparse part   the T x T pre-matrix, the T constants d0 added before partial round 0, then per partial round 2 T + 1
//                 entries (a, b, m00, vhat[T - 1], w[T - 1]), then the field's one          (poseidon_wide_partial_sparse)
// Width 3's table is the dense part alone
H2_HD constexpr uint32_t poseidon_dense_elems(uint32_t t, uint32_t r_f, uint32_t r_p) { return (r_f + r_p) * t + t * t; }
H2_HD constexpr uint32_t poseidon_table_elems(uint32_t t, uint32_t r_f, uint32_t r_p) {
  return poseidon_dense_elems(t, r_f, r_p) + (t == 3 ? 0 : t * t + t + r_p * (2 * t + 1) + 1);
}
// Tree geometry.  log2 of the arity a = width - 1 = 2, 4, 8, and a^e
H2_HD constexpr uint32_t merkle_lg(uint32_t width) { return width == 9 ? 3 : width == 5 ? 2 : 1; }
H2_HD constexpr size_t merkle_pow(uint32_t lg, uint32_t e) { return (size_t)1 << (lg * e); }
// first node of level l (l = 0: the leaves' parents) in the node array of a tree of a^depth leaves: the levels below it hold
// a^(depth-1) + .. + a^(depth-l) = (a^depth - a^(depth-l)) / (a - 1) nodes
H2_HD constexpr size_t merkle_level_offset(uint32_t lg, uint32_t depth, uint32_t l) {
  return (merkle_pow(lg, depth) - merkle_pow(lg, depth - l)) / (((size_t)1 << lg) - 1);
}

// One constant of the table.  The table is not written while a kernel that reads it runs, and the address is the same in
// every lane: on the device the load goes through the constant address space, which the back end always serves with
// scalar loads (for a plain global pointer it does so only where it can prove that no store of the kernel reaches it)
template <class FS>
H2_HD Fe29<FS> poseidon_const(const Fe29<FS>* p) {
#if defined(__HIP_DEVICE_COMPILE__)
  typedef const __attribute__((address_space(4))) int32_t* ConstPtr;
  const ConstPtr q = (ConstPtr)(const int32_t*)p->v;
  Fe29<FS> r;
#pragma unroll
  for (int i = 0; i < 9; i++) r.v[i] = q[i];
  return r;
#else
  return *p;
#endif
}

// x^5 for |x| < c* p (the bounds above): the first squaring is a general product where x^2 may pass fe29_sqr's 64 p^2
template <class FS, class A, int T = 3>
H2_HD Fe29<FS> poseidon_pow5(const Fe29<FS>& x) {
  const Fe29<FS> x2 = T > 5 ? A::template mul<FS>(x, x) : A::template sqr<FS>(x);
  const Fe29<FS> x4 = A::template sqr<FS>(x2);
  return A::template mul<FS>(x4, x);
}
// the S-box input (and, in a dense partial round, the words 1.. as they go into the MDS product): s + rc, carries propagated
template <class FS>
H2_HD Fe29<FS> poseidon_add_rc(const Fe29<FS>& s, const Fe29<FS>* rc) {
  return fe29_norm(fe29_add(s, poseidon_const(rc)));
}

// ---- the width-3 body ------------------------------------------------------------------------------------------------------
// one word of s = M y: three products and two additions, the sum left un-normalised
template <class FS, class A>
H2_HD Fe29<FS> poseidon_mds_row(const Fe29<FS>& y0, const Fe29<FS>& y1, const Fe29<FS>& y2, const Fe29<FS>* row) {
  return fe29_add(fe29_add(A::template mul<FS>(y0, poseidon_const(row)), A::template mul<FS>(y1, poseidon_const(row + 1))),
                  A::template mul<FS>(y2, poseidon_const(row + 2)));
}
template <class FS, class A>
H2_HD void poseidon_permute3(Fe29<FS> s[3], const Fe29<FS>* __restrict__ table, uint32_t r_f, uint32_t r_p) {
  const Fe29<FS>* const mds = table + 3 * (size_t)(r_f + r_p);
  const Fe29<FS>* rc = table;
  const uint32_t half = r_f >> 1;
  Fe29<FS> s0 = s[0], s1 = s[1], s2 = s[2];
#pragma unroll 1
  for (int run = 0; run < 2; run++) {
#pragma unroll 1
    for (uint32_t r = 0; r < half; r++, rc += 3) {
      const Fe29<FS> y0 = poseidon_pow5<FS, A>(poseidon_add_rc(s0, rc + 0));
      const Fe29<FS> y1 = poseidon_pow5<FS, A>(poseidon_add_rc(s1, rc + 1));
      const Fe29<FS> y2 = poseidon_pow5<FS, A>(poseidon_add_rc(s2, rc + 2));
      s0 = poseidon_mds_row<FS, A>(y0, y1, y2, mds);
      s1 = poseidon_mds_row<FS, A>(y0, y1, y2, mds + 3);
      s2 = poseidon_mds_row<FS, A>(y0, y1, y2, mds + 6);
    }
    if (run == 0) {
#pragma unroll 1
      for (uint32_t r = 0; r < r_p; r++, rc += 3) {
        const Fe29<FS> y0 = poseidon_pow5<FS, A>(poseidon_add_rc(s0, rc + 0));
        const Fe29<FS> y1 = poseidon_add_rc(s1, rc + 1);
        const Fe29<FS> y2 = poseidon_add_rc(s2, rc + 2);
        s0 = poseidon_mds_row<FS, A>(y0, y1, y2, mds);
        s1 = poseidon_mds_row<FS, A>(y0, y1, y2, mds + 3);
        s2 = poseidon_mds_row<FS, A>(y0, y1, y2, mds + 6);
      }
    }
  }
  s[0] = fe29_norm(s0);
  s[1] = fe29_norm(s1);
  s[2] = fe29_norm(s2);
}

// ---- the body of the widths 5 and 9 ------------------------------------------------------------------------------------------
// f(I) for the compile-time constants I = FROM .. TO - 1.  The loops over the words of a state are written with it, not as
// `#pragma unroll` loops: an index that is a constant from the start lets the state array be split into registers before
// any loop pass runs, whereas an array that is still indexed by a loop variable then can end up in scratch memory (seen at
// width 9: 336 bytes a lane)
template <int FROM, int TO, class F>
H2_HD void poseidon_wide_each(F&& f) {
  if constexpr (FROM < TO) {
    f(std::integral_constant<int, FROM>());
    poseidon_wide_each<FROM + 1, TO>(f);
  }
}
// s <- (s[1], .., s[T - 1], last).  A recursion over constant indices, as poseidon_wide_each and for its reason
template <class FS, int T, int K = 0>
H2_HD void poseidon_wide_rotate(Fe29<FS> (&s)[T], const Fe29<FS>& last) {
  if constexpr (K + 1 < T) {
#pragma unroll
    for (int l = 0; l < 9; l++) s[K].v[l] = s[K + 1].v[l];
    poseidon_wide_rotate<FS, T, K + 1>(s, last);
  } else {
    s[T - 1] = last;
  }
}
// acc + y m for a sum that counts its units: a carry pass as soon as it holds 4
template <class FS, class A>
H2_HD Fe29<FS> poseidon_wide_term(const Fe29<FS>& acc, int& units, const Fe29<FS>& y, const Fe29<FS>* m) {
  const Fe29<FS> r = fe29_add(acc, A::template mul<FS>(y, poseidon_const(m)));
  if (++units < 4) return r;
  units = 1;
  return fe29_norm(r);
}
// one word of s = M y: T products -> at most 3 units
template <class FS, int T, class A>
H2_HD Fe29<FS> poseidon_wide_row(const Fe29<FS> (&y)[T], const Fe29<FS>* row) {
  Fe29<FS> acc = A::template mul<FS>(y[0], poseidon_const(row));
  int units = 1;
  poseidon_wide_each<1, T>([&](auto j) { acc = poseidon_wide_term<FS, A>(acc, units, y[j], row + j); });
  return acc;
}
// s <- M y, row by row in a loop that stays a loop: row i is appended to s while s rotates, after T trips s[i] = row i
template <class FS, int T, class A>
H2_HD void poseidon_wide_mds(Fe29<FS> (&s)[T], const Fe29<FS> (&y)[T], const Fe29<FS>* mds) {
#pragma unroll 1
  for (int i = 0; i < T; i++) {
    const Fe29<FS> w = poseidon_wide_row<FS, T, A>(y, mds + i * T);
    poseidon_wide_rotate<FS, T>(s, w);
  }
}
// a full round: s <- mat (s + rc)^5.  The S-box runs IN PLACE, one word per trip: the word comes off the front of s, its
// fifth power goes to the back, after T trips s holds the T outputs in order
template <class FS, int T, class A>
H2_HD void poseidon_wide_full_round(Fe29<FS> (&s)[T], const Fe29<FS>* rc, const Fe29<FS>* mat) {
#pragma unroll 1
  for (int j = 0; j < T; j++) {
    const Fe29<FS> p5 = poseidon_pow5<FS, A, T>(poseidon_add_rc(s[0], rc + j));
    poseidon_wide_rotate<FS, T>(s, p5);
  }
  Fe29<FS> o[T];
  poseidon_wide_each<0, T>([&](auto j) { o[j] = Fe29<FS>::zero(); });
  poseidon_wide_mds<FS, T, A>(o, s, mat);
  poseidon_wide_each<0, T>([&](auto j) { s[j] = o[j]; });
}
// the r_p partial rounds, dense: T^2 products each
template <class FS, int T, class A>
H2_HD void poseidon_wide_partial_dense(Fe29<FS> (&s)[T], const Fe29<FS>* rc, const Fe29<FS>* mds, uint32_t r_p) {
  Fe29<FS> y[T];
#pragma unroll 1
  for (uint32_t r = 0; r < r_p; r++, rc += T) {
    y[0] = poseidon_pow5<FS, A, T>(poseidon_add_rc(s[0], rc));
    poseidon_wide_each<1, T>([&](auto j) { y[j] = poseidon_add_rc(s[j], rc + j); });
    poseidon_wide_mds<FS, T, A>(s, y, mds);
  }
}
// the r_p >= 1 partial rounds, sparse: 2 T - 1 products each (the header's "sparse" paragraph).  sp: the sparse part of the
// table behind its pre-matrix.  In: the output of the full round that took the pre-matrix; out: at most 3 units in word 0,
// the other words normalised and below 1.2 p
template <class FS, int T, class A>
H2_HD void poseidon_wide_partial_sparse(Fe29<FS> (&s)[T], const Fe29<FS>* sp, uint32_t r_p) {
  poseidon_wide_each<1, T>([&](auto j) { s[j] = poseidon_add_rc(s[j], sp + j); });
  const Fe29<FS>* const one = sp + T + (size_t)r_p * (2 * T + 1);
  const Fe29<FS>* q = sp + T;
#pragma unroll 1
  for (uint32_t k = 0; k < r_p; k++, q += 2 * T + 1) {
    const Fe29<FS> z = poseidon_add_rc(poseidon_pow5<FS, A, T>(poseidon_add_rc(s[0], q)), q + 1);
    Fe29<FS> acc = A::template mul<FS>(z, poseidon_const(q + 2));
    int units = 1;
    poseidon_wide_each<1, T>([&](auto j) {
      acc = poseidon_wide_term<FS, A>(acc, units, s[j], q + 2 + j);                       // the OLD word j
      s[j] = fe29_norm(fe29_add(s[j], A::template mul<FS>(z, poseidon_const(q + T + 1 + j))));
    });
    s[0] = acc;
    if ((k & (POSEIDON_WIDE_REDUCE_EVERY - 1)) == POSEIDON_WIDE_REDUCE_EVERY - 1 || k + 1 == r_p) {
      poseidon_wide_each<1, T>([&](auto j) { s[j] = A::template mul<FS>(s[j], poseidon_const(one)); });
    }
  }
}
template <class FS, int T, class A, bool SPARSE>
H2_HD void poseidon_permute_wide(Fe29<FS> (&s)[T], const Fe29<FS>* __restrict__ table, uint32_t r_f, uint32_t r_p) {
  const uint32_t half = r_f >> 1;
  const Fe29<FS>* const mds = table + (size_t)T * (r_f + r_p);
  const Fe29<FS>* const sparse = mds + T * T;
  const bool pre = SPARSE && r_p > 0;              // the last full round before the partial ones takes the pre-matrix
  const Fe29<FS>* rc = table;
#pragma unroll 1
  for (int run = 0; run < 2; run++) {              // one full-round body for both runs of full rounds
#pragma unroll 1
    for (uint32_t r = 0; r < half; r++, rc += T)
      poseidon_wide_full_round<FS, T, A>(s, rc, pre && run == 0 && r + 1 == half ? sparse : mds);
    if (run == 0) {
      if constexpr (SPARSE) {
        if (r_p > 0) poseidon_wide_partial_sparse<FS, T, A>(s, sparse + T * T, r_p);
      } else {
        poseidon_wide_partial_dense<FS, T, A>(s, rc, mds, r_p);
      }
      rc += (size_t)T * r_p;
    }
  }
  poseidon_wide_each<0, T>([&](auto j) { s[j] = fe29_norm(s[j]); });
}

// ---- one name for both bodies, and what runs on it -----------------------------------------------------------------------------
// s: T words of at most 3 units and magnitude below (c* - 1) p, c* - 2 for a sponge's state before the absorb (a canonical
// or normalised word is one) -> the permuted state, normalised.  r_f even, r_f + r_p <= POSEIDON_MAX_ROUNDS
template <class FS, int T, class A = Fe29Compiler, bool SPARSE = POSEIDON_SPARSE<T>>
H2_HD void poseidon_permute(Fe29<FS> (&s)[T], const Fe29<FS>* __restrict__ table, uint32_t r_f, uint32_t r_p) {
  static_assert(T == 3 || T == 5 || T == 9, "width 3, 5 or 9");
  static_assert(T != 3 || !SPARSE, "width 3 has the dense table only");
  if constexpr (T == 3) poseidon_permute3<FS, A>(s, table, r_f, r_p);
  else poseidon_permute_wide<FS, T, A, SPARSE>(s, table, r_f, r_p);
}

// ConstantLength<len> at rate T - 1: msg = len canonical elements in the API form; cap = len 2^64 in the working form
template <class FS, int T, class A = Fe29Compiler>
H2_HD Fe29<FS> poseidon_hash(const U128* __restrict__ msg, uint32_t len, const Fe29<FS>& cap, const Fe29<FS>* __restrict__ table,
                             uint32_t r_f, uint32_t r_p) {
  constexpr uint32_t RATE = T - 1;
  Fe29<FS> s[T];
  poseidon_wide_each<0, T - 1>([&](auto j) { s[j] = Fe29<FS>::zero(); });
  s[T - 1] = cap;
#pragma unroll 1
  for (uint32_t off = 0; off < len; off += RATE) {
    // word j at the constant distance 2 j behind word 0's address, so that the loads share one base register: with the sum
    // off + j formed first, in 32 bits, the width-3 kernel computed a second address and came out 5.6 % slower on the Pasta
    // fields (profiles/poseidon_one_family_parent_vs_branch.txt)
    poseidon_wide_each<0, T - 1>([&](auto j) {
      if (off + j < len) s[j] = fe29_add(s[j], fe29_from_api(fe_load<FS>(msg + 2 * (size_t)off + 2 * j)));
    });
    poseidon_permute<FS, T, A>(s, table, r_f, r_p);
  }
  return s[0];
}
// the same on T - 1 words already in the working form (normalised) in s[0 .. T - 2]: a Merkle node from its children
template <class FS, int T, class A = Fe29Compiler>
H2_HD Fe29<FS> poseidon_hash_words(Fe29<FS> (&s)[T], const Fe29<FS>& cap, const Fe29<FS>* __restrict__ table, uint32_t r_f,
                                   uint32_t r_p) {
  s[T - 1] = cap;
  poseidon_permute<FS, T, A>(s, table, r_f, r_p);
  return s[0];
}

#if defined(__HIPCC__)
// n states of T elements (API form), one lane per state; out may be in itself
template <class FS, int T, bool SPARSE>
__global__ void __launch_bounds__(POSEIDON_THREADS)
poseidon_permute_kernel(const U128* in, U128* out, size_t n, const Fe29<FS>* __restrict__ table, uint32_t r_f, uint32_t r_p) {
  const size_t stride = (size_t)gridDim.x * POSEIDON_THREADS;
  for (size_t i = (size_t)blockIdx.x * POSEIDON_THREADS + threadIdx.x; i < n; i += stride) {
    Fe29<FS> s[T];
    poseidon_wide_each<0, T>([&](auto j) { s[j] = fe29_from_api(fe_load<FS>(in + 2 * T * i + 2 * j)); });
    poseidon_permute<FS, T, Fe29Compiler, SPARSE>(s, table, r_f, r_p);
    poseidon_wide_each<0, T>([&](auto j) { fe_store<FS>(out + 2 * T * i + 2 * j, fe29_to_api(s[j])); });
  }
}

// n messages of len elements, msg_stride elements apart -> n elements; one lane per message
template <class FS, int T, class A>
__global__ void __launch_bounds__(POSEIDON_THREADS)
poseidon_hash_kernel(const U128* __restrict__ msgs, uint32_t len, size_t msg_stride, size_t n, U128* __restrict__ out, Fe29<FS> cap,
                     const Fe29<FS>* __restrict__ table, uint32_t r_f, uint32_t r_p) {
  const size_t stride = (size_t)gridDim.x * POSEIDON_THREADS;
  for (size_t i = (size_t)blockIdx.x * POSEIDON_THREADS + threadIdx.x; i < n; i += stride)
    fe_store<FS>(out + 2 * i, fe29_to_api(poseidon_hash<FS, T, A>(msgs + 2 * i * msg_stride, len, cap, table, r_f, r_p)));
}
#endif  // __HIPCC__

}  // namespace h2
