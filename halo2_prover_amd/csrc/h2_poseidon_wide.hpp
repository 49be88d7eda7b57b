// h2_poseidon_wide.hpp -- the Poseidon permutation at WIDTH T = 5 and 9 (rate T - 1 = 4 and 8, S-box x^5), the
// ConstantLength sponge on it and 4-ary / 8-ary Merkle trees of ConstantLength<T - 1> hashes, over the scalar field of a
// curve, on the 9 x 29-bit working form (h2_field29.hpp).  The wide family of include/h2hip.h: h2_poseidon_wide_*.
//
// The same restatement of the reference's primitives.rs as h2_poseidon.hpp (permute :87-132, the sponge :204-390 with the
// capacity word LAST: state (0, .., 0, L 2^64), `rate` words absorbed per permutation, zero-padded, output = word 0), which
// there is generic over Spec<F, T, RATE> and here over the template parameter T.  The judge is oracle/pyref.py, generic
// in t already.  Table in HBM, working form, 36 bytes an entry: (r_f + r_p) x T round constants, then the T x T MDS
// row-major, then the sparse form of the partial rounds (poseidon_wide_table_elems below); read through the constant
// address space (poseidon_const), the round and row index being the same in every lane.  Width 3 is not instantiated: the wide entry points hand width 3 to the calls of h2_poseidon.hpp.
//
// What does not carry over from width 3 is the limb arithmetic of a row.  Write u = 2^29 - 1 and call a word "of k units"
// when its limbs 0..7 lie in [0, k u] (a product's result and a canonical constant are of 1 unit, fe29_add adds units).
//   norm    fe29_norm(a) is safe for a of AT MOST 4 UNITS: the carry into a limb is at most (4 u + 3) >> 29 = 3 and
//           limb + carry <= 4 u + 3 = 2^31 - 1 does not wrap.  A fifth unit (5 u > 2^31) would.  h2_poseidon.hpp sums its three
//           products and the round constant to exactly 4 units; a row of T >= 4 products cannot be summed that way.
//   row     poseidon_wide_row adds the T products one by one and counts units at compile time: whenever the running sum
//           reaches 4 units it is passed through fe29_norm (back to 1 unit), and so is a sum that would END on 4.  The
//           carry passes therefore stand behind the 4th product, then behind every 3rd after it:
//               T = 5:  norm(t0 + t1 + t2 + t3) + t4                               1 pass,  the word has 2 units
//               T = 9:  norm(norm(t0 + t1 + t2 + t3) + t4 + t5 + t6) + t7 + t8     2 passes, the word has 3 units
//           A state word between rounds has at most 3 units, so s + rc has at most 4 and the round's own fe29_norm
//           (poseidon_add_rc, as at width 3) is safe.  The absorbed word of a sponge goes onto a NORMALISED state (1 + 1 units;
//           + rc: 3).  The top limb is signed and small (below 2^26 for any value under 64 p), four of them do not wrap.
//   value   rho = p / R' <= 2^-7 (1 + 2^-127).  A term mul(y, m) with m canonical lies in (-p - |y| rho, |y| rho], so
//           |term| < (1 + c rho) p when |y| <= c p.  A round's input x = s + rc then has |x| < (1 + T (1 + c rho)) p: the map
//           c -> 1 + T (1 + c rho) contracts (T rho < 1) onto its fixed point (1 + T) / (1 - T rho) = 6.25 (T = 5), 10.76
//           (T = 9).  The first round of a sponge permutation sees the normalised output of the last one (|s| < T (1 + c rho)
//           p), a message word below p and a round constant below p.  With c* = fixed point + 1 every round input of every
//           permutation satisfies
//               |x| < c* p,     c* = 7.25 (T = 5),   11.76 (T = 9)
//           (the sequence starts at or below c* and moves towards the fixed point below it), and a permutation's output has
//           |s| < T (1 + c* rho) p = 5.29 p, 9.83 p <= (c* - 2) p: the next absorb closes the loop.
//   S-box   T = 5: x^2 < 52.6 p^2 <= 64 p^2, fe29_sqr's precondition: x2 = sqr(x) in (-p, 0.42 p], x4 = sqr(x2) in
//           (-p, rho p], x5 = mul(x4, x) with |x4 x| < c* p^2: |x5| < (1 + c* rho) p = 1.06 p.
//           T = 9: x^2 < 138.3 p^2 is OUTSIDE fe29_sqr's 64 p^2.  The first squaring is therefore fe29_mul(x, x), whose
//           contract holds for any operands within the limb bounds (x is normalised: limbs below 2^29): x2 in
//           (-p, 1.09 p].  Then x2^2 < 1.2 p^2, x4 = sqr(x2) in (-p, rho p], x5 = mul(x4, x): |x5| < 1.10 p.  Cost: 36
//           limb products more than a squaring, once per S-box -- below 1 % of a permutation.
//   MDS     y is an S-box output (|y| < 1.10 p) or, in a partial round, the normalised x of words 1.. (|y| < c* p): the
//           "value" bound above covers both.  Every operand of every product is normalised on the wide side and canonical or
//           normalised on the narrow side, within fe29_mul's |a_i| < 2^30, |b_j| < 2^29.
//   out     the permutation ends with fe29_norm of every word (at most 3 units): fit for fe29_to_api (|value| < 64 p), for
//           the LDS of the Merkle tail and as the state an absorb adds to.
//
//   sparse  The r_p partial rounds run in the factored form of h2_poseidon_host.hpp (factor_partial_rounds): the full round in
//           front of them takes the pre-matrix in place of the MDS (the bounds of a full round do not depend on the
//           matrix: its entries are canonical), d0 is added to the words 1.. once (s_j + d0_j: 3 + 1 units, normalised, |.| <
//           c* p), and round k is
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
//   kernel is built in both forms and the tests compare them.
//
// Registers and code size.  A width-9 state is 81 limbs and the outputs of a full round's S-boxes another 81.  Unrolling a
// full round over its words and rows would put 3 T + T^2 = 108 inlined products into its body alone (about 2 KB each).
// Instead the words of a full round and the rows of its MDS product are LOOPS kept as loops (#pragma unroll 1) over a register
// array that is ROTATED by one word per trip (poseidon_wide_rotate), so that every index stays a compile-time constant and
// nothing goes to scratch: the S-box loop takes word 0 and appends its fifth power, the row loop computes row i from the T
// outputs (the row's constants at mat + i T, a scalar address) and appends it.  The full-round body holds 3 + T products,
// the sparse partial round 3 + 2 T - 1 and the T - 1 of the reduction.  The price of the rotation: the register allocator
// keeps both ends of the rotating arrays, so the kernels hold 190 - 280 VGPRs at width 5 (two waves per SIMD; one in the
// hash kernel on the compiler's products) and 320 - 500 at width 9 (one wave per SIMD), without scratch.  profiles/poseidon_wide_resources.txt has every kernel,
// DESIGN.md section 7.19 the measurements.
//
// Not here: an in-place update of a wide tree, and a form with several lanes per permutation.
#pragma once
#include <type_traits>

#include "h2_merkle_ops.hpp"
#include "h2_poseidon.hpp"

namespace h2 {

// The table of (T, r_f, r_p), R = r_f + r_p rounds, entries of 36 bytes:
//   dense part    R T round constants, the T x T MDS row-major             (h2_poseidon_wide_constants' elements)
//   sparse part   the T x T pre-matrix, the T constants d0 added before partial round 0, then per partial round 2 T + 1
//                 entries (a, b, m00, vhat[T - 1], w[T - 1]), then the field's one          (poseidon_wide_partial_sparse)
H2_HD constexpr uint32_t poseidon_wide_dense_elems(uint32_t t, uint32_t r_f, uint32_t r_p) { return (r_f + r_p) * t + t * t; }
H2_HD constexpr uint32_t poseidon_wide_sparse_elems(uint32_t t, uint32_t r_p) { return t * t + t + r_p * (2 * t + 1) + 1; }
H2_HD constexpr uint32_t poseidon_wide_table_elems(uint32_t t, uint32_t r_f, uint32_t r_p) {
  return poseidon_wide_dense_elems(t, r_f, r_p) + poseidon_wide_sparse_elems(t, r_p);
}
// The widths whose partial rounds run in the sparse form.  Measured on the permutation kernel (tools/poseidon_wide_bench.py,
// DESIGN.md section 7.19); the permutation kernel alone is also built in the other form, for that measurement and the tests
template <int T>
constexpr bool POSEIDON_WIDE_SPARSE = true;
// partial rounds between two value reductions of the words 1.. in the sparse form (a power of two)
constexpr uint32_t POSEIDON_WIDE_REDUCE_EVERY = 8;
// a^e for the arities 2, 4, 8 (lg = 1, 2, 3)
H2_HD constexpr size_t merkle_wide_pow(uint32_t lg, uint32_t e) { return (size_t)1 << (lg * e); }
// first node of level l (l = 0: the leaves' parents) in the node array of a tree of a^depth leaves: the levels below it hold
// a^(depth-1) + .. + a^(depth-l) = (a^depth - a^(depth-l)) / (a - 1) nodes
H2_HD constexpr size_t merkle_wide_level_offset(uint32_t lg, uint32_t depth, uint32_t l) {
  return (merkle_wide_pow(lg, depth) - merkle_wide_pow(lg, depth - l)) / (((size_t)1 << lg) - 1);
}

// x^5 for |x| < c* p (the bounds above): the first squaring is a general product where x^2 may pass fe29_sqr's 64 p^2
template <class FS, int T, class A>
H2_HD Fe29<FS> poseidon_wide_pow5(const Fe29<FS>& x) {
  const Fe29<FS> x2 = T > 5 ? A::template mul<FS>(x, x) : A::template sqr<FS>(x);
  const Fe29<FS> x4 = A::template sqr<FS>(x2);
  return A::template mul<FS>(x4, x);
}
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
    const Fe29<FS> p5 = poseidon_wide_pow5<FS, T, A>(poseidon_add_rc(s[0], rc + j));
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
    y[0] = poseidon_wide_pow5<FS, T, A>(poseidon_add_rc(s[0], rc));
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
    const Fe29<FS> z = poseidon_add_rc(poseidon_wide_pow5<FS, T, A>(poseidon_add_rc(s[0], q)), q + 1);
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

// s: T words of at most 3 units and magnitude below (c* - 1) p, c* - 2 for a sponge's state before the absorb (a canonical
// or normalised word is one) -> the permuted state, normalised.  r_f even, r_f + r_p <= POSEIDON_MAX_ROUNDS
template <class FS, int T, class A = Fe29Compiler, bool SPARSE = POSEIDON_WIDE_SPARSE<T>>
H2_HD void poseidon_wide_permute(Fe29<FS> (&s)[T], const Fe29<FS>* __restrict__ table, uint32_t r_f, uint32_t r_p) {
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

// ConstantLength<len> at rate T - 1: msg = len canonical elements in the API form; cap = len 2^64 in the working form
template <class FS, int T, class A = Fe29Compiler>
H2_HD Fe29<FS> poseidon_wide_hash(const U128* __restrict__ msg, uint32_t len, const Fe29<FS>& cap, const Fe29<FS>* __restrict__ table,
                                  uint32_t r_f, uint32_t r_p) {
  constexpr uint32_t RATE = T - 1;
  Fe29<FS> s[T];
  poseidon_wide_each<0, T - 1>([&](auto j) { s[j] = Fe29<FS>::zero(); });
  s[T - 1] = cap;
#pragma unroll 1
  for (uint32_t off = 0; off < len; off += RATE) {
    poseidon_wide_each<0, T - 1>([&](auto j) {
      if (off + j < len) s[j] = fe29_add(s[j], fe29_from_api(fe_load<FS>(msg + 2 * (size_t)(off + j))));
    });
    poseidon_wide_permute<FS, T, A>(s, table, r_f, r_p);
  }
  return s[0];
}
// the same on T - 1 words already in the working form (normalised) in s[0 .. T - 2]: a Merkle node from its children
template <class FS, int T, class A = Fe29Compiler>
H2_HD Fe29<FS> poseidon_wide_hash_words(Fe29<FS> (&s)[T], const Fe29<FS>& cap, const Fe29<FS>* __restrict__ table, uint32_t r_f,
                                        uint32_t r_p) {
  s[T - 1] = cap;
  poseidon_wide_permute<FS, T, A>(s, table, r_f, r_p);
  return s[0];
}

#if defined(__HIPCC__)
// n states of T elements (API form), one lane per state; out may be in itself
template <class FS, int T, bool SPARSE>
__global__ void __launch_bounds__(POSEIDON_THREADS)
poseidon_wide_permute_kernel(const U128* in, U128* out, size_t n, const Fe29<FS>* __restrict__ table, uint32_t r_f, uint32_t r_p) {
  const size_t stride = (size_t)gridDim.x * POSEIDON_THREADS;
  for (size_t i = (size_t)blockIdx.x * POSEIDON_THREADS + threadIdx.x; i < n; i += stride) {
    Fe29<FS> s[T];
    poseidon_wide_each<0, T>([&](auto j) { s[j] = fe29_from_api(fe_load<FS>(in + 2 * T * i + 2 * j)); });
    poseidon_wide_permute<FS, T, Fe29Compiler, SPARSE>(s, table, r_f, r_p);
    poseidon_wide_each<0, T>([&](auto j) { fe_store<FS>(out + 2 * T * i + 2 * j, fe29_to_api(s[j])); });
  }
}

// n messages of len elements, msg_stride elements apart -> n elements; one lane per message
template <class FS, int T, class A>
__global__ void __launch_bounds__(POSEIDON_THREADS)
poseidon_wide_hash_kernel(const U128* __restrict__ msgs, uint32_t len, size_t msg_stride, size_t n, U128* __restrict__ out, Fe29<FS> cap,
                          const Fe29<FS>* __restrict__ table, uint32_t r_f, uint32_t r_p) {
  const size_t stride = (size_t)gridDim.x * POSEIDON_THREADS;
  for (size_t i = (size_t)blockIdx.x * POSEIDON_THREADS + threadIdx.x; i < n; i += stride)
    fe_store<FS>(out + 2 * i, fe29_to_api(poseidon_wide_hash<FS, T, A>(msgs + 2 * i * msg_stride, len, cap, table, r_f, r_p)));
}

// The top of an a-ary tree (a = T - 1) in ONE workgroup: `width` nodes (a power of a, 1 <= width <=
// POSEIDON_MERKLE_TAIL_MAX) from their a width children at `in`, then every level above them up to the root, each level
// written behind the one before at `out`.  As poseidon_merkle_tail_kernel: the levels above the first are read from LDS in
// the working form, two buffers alternate, a barrier separates a level's writes from the next level's reads.  Limb-major:
// lane i's limb l at [l][i].  The first level goes to lvl_a (up to TAIL_MAX nodes), the second to lvl_b (up to TAIL_MAX / a)
template <class FS, int T>
__global__ void __launch_bounds__(POSEIDON_THREADS)
poseidon_wide_merkle_tail_kernel(const U128* __restrict__ in, U128* __restrict__ out, uint32_t width, Fe29<FS> cap,
                                 const Fe29<FS>* __restrict__ table, uint32_t r_f, uint32_t r_p) {
  constexpr uint32_t ARITY = T - 1;
  __shared__ int32_t lvl_a[9 * POSEIDON_MERKLE_TAIL_MAX];
  __shared__ int32_t lvl_b[9 * (POSEIDON_MERKLE_TAIL_MAX / ARITY)];
  const uint32_t t = threadIdx.x;
  int32_t* src = lvl_b;
  int32_t* dst = lvl_a;
  uint32_t src_ld = POSEIDON_MERKLE_TAIL_MAX / ARITY, dst_ld = POSEIDON_MERKLE_TAIL_MAX;
  bool first = true;
#pragma unroll 1
  for (uint32_t w = width; w >= 1; w /= ARITY) {
    for (uint32_t i = t; i < w; i += POSEIDON_THREADS) {
      Fe29<FS> s[T];
      if (first) {
        poseidon_wide_each<0, T - 1>([&](auto c) { s[c] = fe29_from_api(fe_load<FS>(in + 2 * ((size_t)ARITY * i + c))); });
      } else {
        poseidon_wide_each<0, T - 1>([&](auto c) {
#pragma unroll
          for (int l = 0; l < 9; l++) s[c].v[l] = src[l * src_ld + ARITY * i + c];
        });
      }
      const Fe29<FS> h = poseidon_wide_hash_words<FS, T, Fe29Compiler>(s, cap, table, r_f, r_p);
#pragma unroll
      for (int l = 0; l < 9; l++) dst[l * dst_ld + i] = h.v[l];
      fe_store<FS>(out + 2 * (size_t)i, fe29_to_api(h));
    }
    __syncthreads();
    out += 2 * (size_t)w;
    int32_t* const tp = src; src = dst; dst = tp;
    const uint32_t tl = src_ld; src_ld = dst_ld; dst_ld = tl;
    first = false;
  }
}

// ---- paths: a gather --------------------------------------------------------------------------------------------------
// one lane per (item, level, sibling): paths[i][l][k] = child c of the parent of leaf indices[i]'s ancestor at level l, c
// running over the parent's a = 2^lg children in order with the ancestor's own position left out; zero when the index is
// out of range.  The index is checked against a^depth before it addresses anything
static __global__ void __launch_bounds__(POSEIDON_THREADS)
poseidon_wide_merkle_paths_kernel(const U128* __restrict__ leaves, const U128* __restrict__ nodes, uint32_t lg, uint32_t depth,
                                  const uint32_t* __restrict__ indices, size_t n, U128* __restrict__ paths,
                                  uint32_t* __restrict__ status) {
  const uint32_t sibs = (1u << lg) - 1, per_item = depth * sibs;
  const size_t stride = (size_t)gridDim.x * POSEIDON_THREADS, total = n * per_item;
  for (size_t t = (size_t)blockIdx.x * POSEIDON_THREADS + threadIdx.x; t < total; t += stride) {
    const size_t i = t / per_item;
    const uint32_t e = (uint32_t)(t - i * per_item), l = e / sibs, k = e - l * sibs, idx = indices[i];
    const bool ok = idx < ((uint32_t)1 << (lg * depth));
    U128 lo = U128{0, 0, 0, 0}, hi = lo;
    if (ok) {
      const uint32_t node = idx >> (lg * l), pos = node & sibs;
      const size_t sib = (size_t)((node & ~sibs) | (k < pos ? k : k + 1));
      const U128* src = l == 0 ? leaves + 2 * sib : nodes + 2 * (merkle_wide_level_offset(lg, depth, l - 1) + sib);
      lo = src[0];
      hi = src[1];
    }
    paths[2 * t] = lo;
    paths[2 * t + 1] = hi;
    if (e == 0) status[i] = ok ? MERKLE_OK : MERKLE_RANGE;
  }
}

// ---- verify: one lane per path ------------------------------------------------------------------------------------------
// cur = leaf; per level the a words are the level's a - 1 siblings with cur inserted at its position, cur = their hash; the
// value stays in the working form between levels.  An index out of range (status 1) or an element that is not canonical
// (status 2) ends the item with a zero root before any product sees it.  root: null, or the element every computed root is
// compared with
template <class FS, int T>
__global__ void __launch_bounds__(POSEIDON_THREADS)
poseidon_wide_merkle_verify_kernel(const U128* __restrict__ leaf_values, const uint32_t* __restrict__ indices,
                                   const U128* __restrict__ paths, uint32_t depth, size_t n, const U128* __restrict__ root,
                                   U128* __restrict__ roots_out, uint32_t* __restrict__ status, Fe29<FS> cap,
                                   const Fe29<FS>* __restrict__ table, uint32_t r_f, uint32_t r_p) {
  constexpr uint32_t ARITY = T - 1, SIBS = ARITY - 1, LG = ARITY == 8 ? 3 : ARITY == 4 ? 2 : 1;
  static_assert(ARITY == (1u << LG), "arity 2, 4 or 8");
  const size_t stride = (size_t)gridDim.x * POSEIDON_THREADS;
  for (size_t i = (size_t)blockIdx.x * POSEIDON_THREADS + threadIdx.x; i < n; i += stride) {
    const uint32_t idx = indices[i];
    const Fe<FS> leaf = fe_load<FS>(leaf_values + 2 * i);
    uint32_t st = idx < ((uint32_t)1 << (LG * depth)) ? MERKLE_OK : MERKLE_RANGE;
    if (st == MERKLE_OK && !fe_is_canonical(leaf)) st = MERKLE_NONCANONICAL;
    Fe29<FS> cur = fe29_from_api(leaf);
    const U128* path = paths + 2 * i * depth * SIBS;
#pragma unroll 1
    for (uint32_t l = 0; l < depth && st == MERKLE_OK; l++) {
      const uint32_t pos = (idx >> (LG * l)) & SIBS;
      Fe29<FS> s[T];
      poseidon_wide_each<0, T - 1>([&](auto ci) {
        constexpr uint32_t c = (uint32_t)decltype(ci)::value;
        // child c: cur at its own position, else sibling c (before it) or c - 1 (behind it).  k <= SIBS - 1 either way: the
        // load that position `pos` does not need stays inside the level's siblings
        const uint32_t k = c < pos ? c : c == 0 ? 0 : c - 1;
        const Fe<FS> sib = fe_load<FS>(path + 2 * ((size_t)l * SIBS + k));
        if (c != pos && !fe_is_canonical(sib)) st = MERKLE_NONCANONICAL;
        s[c] = fe29_from_api(sib);
        if (c == pos) s[c] = cur;
      });
      if (st != MERKLE_OK) break;
      cur = poseidon_wide_hash_words<FS, T, Fe29Compiler>(s, cap, table, r_f, r_p);
    }
    Fe<FS> r;
#pragma unroll
    for (int j = 0; j < 8; j++) r.v[j] = 0;
    if (st == MERKLE_OK) {
      r = fe29_to_api(cur);
      if (root) {
        const Fe<FS> want = fe_load<FS>(root);
        uint32_t diff = 0;
#pragma unroll
        for (int j = 0; j < 8; j++) diff |= r.v[j] ^ want.v[j];
        if (diff) st = MERKLE_MISMATCH;
      }
    }
    if (roots_out) fe_store<FS>(roots_out + 2 * i, r);
    status[i] = st;
  }
}
#endif  // __HIPCC__

}  // namespace h2
