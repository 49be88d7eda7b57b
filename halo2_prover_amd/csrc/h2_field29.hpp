// h2_field29.hpp -- the MSM's working representation of base-field elements: 9 signed limbs of 29 bits,
// Montgomery form with R' = 2^261, values kept only loosely reduced.
//
// Why (measured, tools/microbench_limb29.hip -> profiles/r01_microbench_limb29.txt): on 8 x 32-bit limbs every
// v_mad_u64_u32 of the Montgomery product needs a v_addc_co_u32 to count the carry out of its 64-bit column and the
// column hand-over costs three moves (h2_field.hpp, fe_mul_comba).  A column of 29-bit limb products -- at most nine
// a_i b_j and nine m_i p_j -- cannot overflow 64 bits, so there is no carry counter, the hand-over is one shift, and
// because R' is 2^7 times the modulus there is no conditional subtraction either.  Price: 81 + 9 k multiply-adds
// (k = non-trivial modulus limbs: 4 for the Pasta primes, 9 for BN254) instead of 64 + 8 k'.  Result on MI355X:
// 167 against 122 G modmul/s with four waves per SIMD, 144 against 88 for a lone wave (Pasta Fp).
//
// Invariants (the callers in h2_curve29.hpp are written against these):
//   value   x R' mod p, as the integer  sum_i v[i] 2^(29 i)  with SIGNED limbs -- it may be negative or exceed p.
//   fe29_mul(a, b): needs only the limb bounds |a_i| < 2^30 and |b_j| < 2^29 (or the other way round: the sums of 18
//           limb products must stay below 2^63).  Returns exactly (a b - m p) / R' with m = a b p^-1 mod R', 0 <= m < R'
//           (the SUBTRACTIVE reduction, below), in the normalised form: limbs 0..7 in [0, 2^29), the top limb signed.
//           Its value lies in (a b / R' - p, a b / R'] for ANY operands within the limb bounds (tests/
//           test_fe29_product.py checks products up to 1024 p^2: the callers' (+-32 p)^2 in expr_kernel, (+-16 p)^2 in
//           perm_ratio_kernel).  Only when also |a| |b| <= 64 p^2 is it in (-3p/2, p/2] -- the mirror image of the
//           additive form's (-p/2, 3p/2), so every magnitude bound the callers were written against (|x| < 1.5p for a
//           product of such operands) still holds; only what relied on the sign moved (fe29_canonical_pack,
//           fe29_to_api, w_canonical_pack; the NTT's inter-pass store keeps the additive fe29_mul_up, exactly
//           (a b + m' p) / R' with m' = -a b p^-1 mod R', in [a b / R', a b / R' + p)).  For the Pasta primes
//           64 p / R' exceeds 1/2 by 2^-127 relative, so "p/2" there means p/2 (1 + 2^-127); nothing below depends on
//           that slack.
//   fe29_sqr(a): |a_i| < 2^29, |a|^2 <= 64 p^2; fe29_mul_sub(a, b, c, d): every limb below 2^29 in magnitude,
//           |a b - c d| <= 64 p^2.  Same output limbs and range as fe29_mul.
//   fe29_add / fe29_sub / fe29_neg: limb-wise, no carries: limb magnitudes add up.  A difference of two normalised
//           values has limbs of magnitude < 2^29 and can go straight into a product; anything built from three or
//           more terms is passed through fe29_norm (carry propagation: limbs back in [0, 2^29), value unchanged).
//   exact zero (all limbs 0) only ever arises from the identity's coordinates, so `is_zero_exact` is the identity
//   test; `fe29_is_zero_mod_p` is the real test for the exceptional cases of the addition formulas.
//
// The column kernel (round 4): each column is its limb products as 64-bit multiply-adds, then the Montgomery step
// m = acc p^-1 mod 2^29 and acc -= m p.  For p = 1 mod 2^29 (Pasta) m is acc's low 29 bits and the p[0] term is never
// computed (acc - m only clears what the arithmetic shift drops); the top limb 2^22 is one multiply-add with a hidden
// constant instead of a 64-bit shift and add.  What is left per column is one AND, one 64-bit shift and the one 64-bit
// add the compiler uses to join the column's two multiply-add chains (the ISA table).  The two
// kernels in which several waves share a SIMD (msm_chunk_kernel, the NTT pass) take the same products from
// h2_field29_chain.hpp instead: one chain per column fixed in asm statements, no join, the same nine limbs.
//
// Conversions need no new constants: the API form x 2^256 is the R' form of x / 32, so going in is five doublings
// in the 32-bit-limb field, and going out is one product with FP::ONE (= 2^256 mod p) read as a plain integer.
#pragma once
#include "h2_field.hpp"

namespace h2 {

constexpr uint32_t L29_MASK = (1u << 29) - 1;

template <class FP>
struct Fe29 {
  int32_t v[9];
  static H2_HD Fe29 zero() {
    Fe29 r;
#pragma unroll
    for (int i = 0; i < 9; i++) r.v[i] = 0;
    return r;
  }
  H2_HD bool is_zero_exact() const {
    int32_t o = 0;
#pragma unroll
    for (int i = 0; i < 9; i++) o |= v[i];
    return o == 0;
  }
};

// limb j (29 bits) of the modulus, from its 32-bit limbs
template <class FP>
H2_HD constexpr uint32_t fe29_p(int j) {
  const int bit = 29 * j;
  const int w = bit / 32, s = bit % 32;
  const uint64_t lo = w < 8 ? FP::P(w) : 0, hi = w + 1 < 8 ? FP::P(w + 1) : 0;
  return (uint32_t)(((lo | (hi << 32)) >> s) & L29_MASK);
}

// 8 x 32 bits (a non-negative integer below 2^256) -> 9 x 29 bits
template <class FP>
H2_HD Fe29<FP> fe29_unpack(const Fe<FP>& a) {
  Fe29<FP> r;
#pragma unroll
  for (int j = 0; j < 9; j++) {
    const int bit = 29 * j, w = bit >> 5, s = bit & 31;
    const uint64_t lo = a.v[w], hi = w + 1 < 8 ? a.v[w + 1] : 0;
    r.v[j] = (int32_t)((uint32_t)((lo | (hi << 32)) >> s) & L29_MASK);
  }
  return r;
}
// 9 normalised limbs of a non-negative integer below 2^256 -> 8 x 32 bits
template <class FP>
H2_HD Fe<FP> fe29_pack(const Fe29<FP>& a) {
  Fe<FP> r;
#pragma unroll
  for (int w = 0; w < 8; w++) {
    const int bit = 32 * w, j = bit / 29, off = bit % 29;
    uint64_t x = (uint64_t)(uint32_t)a.v[j] >> off;
    x |= (uint64_t)(uint32_t)a.v[j + 1] << (29 - off);
    if (j + 2 < 9) x |= (uint64_t)(uint32_t)a.v[j + 2] << (58 - off);
    r.v[w] = (uint32_t)x;
  }
  return r;
}

template <class FP>
H2_HD Fe29<FP> fe29_add(const Fe29<FP>& a, const Fe29<FP>& b) {
  Fe29<FP> r;
#pragma unroll
  for (int i = 0; i < 9; i++) r.v[i] = a.v[i] + b.v[i];
  return r;
}
template <class FP>
H2_HD Fe29<FP> fe29_sub(const Fe29<FP>& a, const Fe29<FP>& b) {
  Fe29<FP> r;
#pragma unroll
  for (int i = 0; i < 9; i++) r.v[i] = a.v[i] - b.v[i];
  return r;
}
template <class FP>
H2_HD Fe29<FP> fe29_neg(const Fe29<FP>& a) {
  Fe29<FP> r;
#pragma unroll
  for (int i = 0; i < 9; i++) r.v[i] = -a.v[i];
  return r;
}
// carry propagation: same value, limbs 0..7 in [0, 2^29), the top limb takes the sign
template <class FP>
H2_HD Fe29<FP> fe29_norm(const Fe29<FP>& a) {
  Fe29<FP> r;
  int32_t carry = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const int32_t x = a.v[i] + carry;
    r.v[i] = (int32_t)((uint32_t)x & L29_MASK);
    carry = x >> 29;                      // arithmetic
  }
  r.v[8] = a.v[8] + carry;
  return r;
}

// The limb products are signed 32 x 32 -> 64 multiply-adds: ONE v_mad_i64_i32 each.  But where the optimiser can PROVE a
// limb non-negative (a value just unpacked or masked) it rewrites that operand's sign extension as a zero extension,
// and the back end then has neither its signed nor its unsigned pattern for sext(a) * zext(b): it multiplies 32 x 64
// bits -- two v_mad_u64_u32, two moves, and for the signed top limbs two v_mul_lo_u32 and a v_add3_u32 more (seen in
// msm_chunk_kernel's ISA: 1211 multiply-adds + 112 v_mul_lo_u32 per point addition against 1062 limb products).  An
// empty asm statement per operand limb hides the range from the optimiser and costs no instruction.
H2_HD int32_t fe29_opaque(int32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
  asm("" : "+v"(x));
#endif
  return x;
}
namespace detail29 {
// a constant the optimiser may not see (it stays in a scalar register): m * 2^22 or m * (2^28 + 1) is then ONE
// multiply-add, not the 64-bit shifts and 64-bit adds the optimiser would rewrite it into
H2_HD int32_t fe29_hidden(int32_t c) {
#if defined(__HIP_DEVICE_COMPILE__)
  asm("" : "+s"(c));
#endif
  return c;
}
// acc -= m * p[J]: a zero limb costs nothing, every other one (2^22 included) one multiply-add with -p[J]; the sparse
// constants are hidden, the dense ones are not worth a shift sequence to the optimiser anyway.  UP (the additive form,
// fe29_mul_up): acc += m * p[J], the constant limb folded: 1 -> add, 2^s -> shifted add
template <class FP, int J, bool UP>
H2_HD void msub_p(int64_t& acc, int32_t m) {
  constexpr uint32_t pj = fe29_p<FP>(J);
  if constexpr (UP) {
    if constexpr (pj == 0) {
    } else if constexpr (pj == 1) {
      acc += m;
    } else if constexpr ((pj & (pj - 1)) == 0) {
      acc += (int64_t)m << __builtin_ctz(pj);
    } else {
      acc += (int64_t)m * (int32_t)pj;
    }
  } else if constexpr (pj == 0) {
  } else if constexpr (__builtin_popcount(pj) <= 2) {
    acc += (int64_t)m * fe29_hidden(-(int32_t)pj);
  } else {
    acc += (int64_t)m * -(int32_t)pj;
  }
}
// the Montgomery step of column K < 9, SUBTRACTIVE: m = acc p^-1 mod 2^29 in [0, 2^29), acc -= m p[0].  For the Pasta
// primes p = 1 mod 2^29: m is acc's own low 29 bits (one AND, no negation, no v_mul_lo_u32) and acc - m p[0] = acc - m
// only clears the bits that the shift after it drops -- the p[0] term is not computed at all
// UP: m = -acc p^-1 mod 2^29 and acc += m p[0] (the form before the subtractive one, kept for fe29_mul_up)
template <class FP, bool UP>
H2_HD int32_t mont_step(int64_t& acc) {
  constexpr uint32_t pinv = (0u - (FP::INV & L29_MASK)) & L29_MASK;     // p^-1 mod 2^29 (FP::INV = -p^-1 mod 2^32)
  if constexpr (UP) {
    constexpr uint32_t ninv = FP::INV & L29_MASK;
    const int32_t m = ninv == L29_MASK ? (int32_t)((0u - (uint32_t)acc) & L29_MASK)
                                       : (int32_t)(((uint32_t)acc * ninv) & L29_MASK);
    msub_p<FP, 0, true>(acc, m);
    return m;
  } else if constexpr (pinv == 1) {
    return fe29_opaque((int32_t)((uint32_t)acc & L29_MASK));
  } else {
    const int32_t m = fe29_opaque((int32_t)(((uint32_t)acc * pinv) & L29_MASK));
    msub_p<FP, 0, false>(acc, m);
    return m;
  }
}
template <class FP, int K, int I, int IEND>
H2_HD void col_ab(int64_t& acc, const int32_t* a, const int32_t* b) {
  if constexpr (I <= IEND) {
    acc += (int64_t)a[I] * b[K - I];
    col_ab<FP, K, I + 1, IEND>(acc, a, b);
  }
}
template <class FP, int K, int I, int IEND, bool UP>
H2_HD void col_mp(int64_t& acc, const int32_t* m) {
  if constexpr (I <= IEND) {
    msub_p<FP, K - I, UP>(acc, m[I]);
    col_mp<FP, K, I + 1, IEND, UP>(acc, m);
  }
}
// after column K's limb products: the m p terms, then (K < 9) m[K] such that the column's low 29 bits vanish, or
// (K >= 9) output limb K - 9; the arithmetic shift hands the rest to column K + 1 (exact below K = 9)
template <class FP, int K, bool UP = false>
H2_HD void reduce_col(int64_t& acc, int32_t* m, int32_t* t) {
  if constexpr (K < 9) {
    if constexpr (K > 0) col_mp<FP, K, 0, K - 1, UP>(acc, m);
    m[K] = mont_step<FP, UP>(acc);
  } else {
    col_mp<FP, K, K - 8, 8, UP>(acc, m);
    t[K - 9] = (int32_t)((uint32_t)acc & L29_MASK);
  }
  acc >>= 29;
}
// column K of a*b - m*p (UP: a*b + m*p)
template <class FP, int K, bool UP = false>
H2_HD void columns(int64_t& acc, const int32_t* a, const int32_t* b, int32_t* m, int32_t* t) {
  if constexpr (K < 17) {
    col_ab<FP, K, (K < 9 ? 0 : K - 8), (K < 9 ? K : 8)>(acc, a, b);
    reduce_col<FP, K, UP>(acc, m, t);
    columns<FP, K + 1, UP>(acc, a, b, m, t);
  }
}
// column K of a^2: cross terms with the doubled operand, the square of the middle limb once
template <class FP, int K, int I, int IEND>
H2_HD void col_sq(int64_t& acc, const int32_t* a, const int32_t* a2) {
  if constexpr (I <= IEND) {
    if constexpr (I < K - I) acc += (int64_t)a[I] * a2[K - I];
    else if constexpr (I == K - I) acc += (int64_t)a[I] * a[I];
    col_sq<FP, K, I + 1, IEND>(acc, a, a2);
  }
}
template <class FP, int K>
H2_HD void columns_sq(int64_t& acc, const int32_t* a, const int32_t* a2, int32_t* m, int32_t* t) {
  if constexpr (K < 17) {
    col_sq<FP, K, (K < 9 ? 0 : K - 8), K / 2>(acc, a, a2);
    reduce_col<FP, K>(acc, m, t);
    columns_sq<FP, K + 1>(acc, a, a2, m, t);
  }
}
// column K of a b + c d
template <class FP, int K>
H2_HD void columns2(int64_t& acc, const int32_t* a, const int32_t* b, const int32_t* c, const int32_t* d, int32_t* m, int32_t* t) {
  if constexpr (K < 17) {
    col_ab<FP, K, (K < 9 ? 0 : K - 8), (K < 9 ? K : 8)>(acc, a, b);
    col_ab<FP, K, (K < 9 ? 0 : K - 8), (K < 9 ? K : 8)>(acc, c, d);
    reduce_col<FP, K>(acc, m, t);
    columns2<FP, K + 1>(acc, a, b, c, d, m, t);
  }
}
}  // namespace detail29

template <class FP>
H2_HD void fe29_opaque_limbs(int32_t* o, const Fe29<FP>& a) {
#pragma unroll
  for (int i = 0; i < 9; i++) o[i] = fe29_opaque(a.v[i]);
}

// a b / R' (see the invariants at the top)
template <class FP>
H2_HD Fe29<FP> fe29_mul(const Fe29<FP>& a, const Fe29<FP>& b) {
  int64_t acc = 0;
  int32_t m[9], av[9], bv[9];
  fe29_opaque_limbs(av, a);
  fe29_opaque_limbs(bv, b);
  Fe29<FP> r;
  detail29::columns<FP, 0>(acc, av, bv, m, r.v);
  r.v[8] = (int32_t)acc;
  return r;
}
// the same product with the limbs' ranges left visible to the optimiser (the ceiling microbenchmark times both forms
// and reports the faster: on two operands it knows to be non-negative the compiler picks v_mad_u64_u32 throughout)
template <class FP>
H2_HD Fe29<FP> fe29_mul_plain(const Fe29<FP>& a, const Fe29<FP>& b) {
  int64_t acc = 0;
  int32_t m[9];
  Fe29<FP> r;
  detail29::columns<FP, 0>(acc, a.v, b.v, m, r.v);
  r.v[8] = (int32_t)acc;
  return r;
}
// a b / R' rounded UP: (a b + m p) / R' in [a b / R', a b / R' + p) -- non-negative for a b >= 0.  The form of the
// product before the subtractive one (p[0] and 2^22 terms as 64-bit adds, a negated m): where a non-negative result is
// stored as it is (the NTT's inter-pass product) it costs less than a carry pass after the subtractive product.  (The
// NTT pass itself takes it from h2_field29_chain.hpp where that form exists: there the p[0] and 2^22 terms are
// multiply-adds of the column's one chain, 135 of them and no 64-bit add, still less than the carry pass.)
template <class FP>
H2_HD Fe29<FP> fe29_mul_up(const Fe29<FP>& a, const Fe29<FP>& b) {
  int64_t acc = 0;
  int32_t m[9], av[9], bv[9];
  fe29_opaque_limbs(av, a);
  fe29_opaque_limbs(bv, b);
  Fe29<FP> r;
  detail29::columns<FP, 0, true>(acc, av, bv, m, r.v);
  r.v[8] = (int32_t)acc;
  return r;
}
// a^2 / R': the cross terms a_i a_j (i < j) once, against the doubled limbs 2 a_j -- 45 limb products instead of 81.
// Needs |a_i| < 2^29 (what fe29_mul(a, a) needs): a column is at most four cross terms below 2^59, one square below
// 2^58 and nine m p terms below 2^58, under 2^63.
template <class FP>
H2_HD Fe29<FP> fe29_sqr(const Fe29<FP>& a) {
  int64_t acc = 0;
  int32_t m[9], av[9], a2[9];
  fe29_opaque_limbs(av, a);
#pragma unroll
  for (int i = 0; i < 9; i++) a2[i] = fe29_opaque(av[i] * 2);
  Fe29<FP> r;
  detail29::columns_sq<FP, 0>(acc, av, a2, m, r.v);
  r.v[8] = (int32_t)acc;
  return r;
}
// (a b - c d) / R' with ONE reduction: both products are accumulated column by column before m is chosen (saves the 9 k
// multiply-adds and the carry chain of a second reduction).  Needs every limb below 2^29 in magnitude: a column is at
// most 18 limb products and nine m p terms below 2^58 each, under 2^63; |a b - c d| <= 64 p^2 as for a single product.
template <class FP>
H2_HD Fe29<FP> fe29_mul_sub(const Fe29<FP>& a, const Fe29<FP>& b, const Fe29<FP>& c, const Fe29<FP>& d) {
  int64_t acc = 0;
  int32_t m[9], av[9], bv[9], nc[9], dv[9];
  fe29_opaque_limbs(av, a);
  fe29_opaque_limbs(bv, b);
  fe29_opaque_limbs(dv, d);
#pragma unroll
  for (int i = 0; i < 9; i++) nc[i] = fe29_opaque(-c.v[i]);
  Fe29<FP> r;
  detail29::columns2<FP, 0>(acc, av, bv, nc, dv, m, r.v);
  r.v[8] = (int32_t)acc;
  return r;
}

// API form (x 2^256 mod p, canonical) -> working form (x 2^261 mod p, canonical, normalised limbs)
template <class FP>
H2_HD Fe29<FP> fe29_from_api(const Fe<FP>& a) {
  Fe<FP> t = a;
#pragma unroll
  for (int i = 0; i < 5; i++) t = fe_dbl(t);
  return fe29_unpack(t);
}
// t in (-2p, p) with normalised limbs (a product's result) -> canonical, packed
template <class FP>
H2_HD Fe<FP> fe29_canonical_pack(Fe29<FP> t) {
  Fe29<FP> pl;
#pragma unroll
  for (int i = 0; i < 9; i++) pl.v[i] = (int32_t)fe29_p<FP>(i);
  if (t.v[8] < 0) t = fe29_norm(fe29_add(t, pl));
  if (t.v[8] < 0) t = fe29_norm(fe29_add(t, pl));
  return fe29_pack(t);
}
// working form (any value of magnitude < 64 p, limbs of magnitude < 2^30) -> API form, canonical
template <class FP>
H2_HD Fe<FP> fe29_to_api(const Fe29<FP>& a) {
  Fe<FP> one;
#pragma unroll
  for (int i = 0; i < 8; i++) one.v[i] = FP::ONE(i);                 // 2^256 mod p as a plain integer
  return fe29_canonical_pack(fe29_mul(a, fe29_unpack(one)));        // in (-3p/2, p/2], limbs normalised
}
// t in (-2p, 2p), any limbs within fe29_norm's reach -> canonical, packed (the API's bytes when t is x 2^256 + j p)
template <class FP>
H2_HD Fe<FP> w_canonical_pack(const Fe29<FP>& t0) {
  Fe29<FP> pl;
#pragma unroll
  for (int i = 0; i < 9; i++) pl.v[i] = (int32_t)fe29_p<FP>(i);
  Fe29<FP> t = fe29_norm(t0);
  if (t.v[8] < 0) t = fe29_norm(fe29_add(t, pl));
  if (t.v[8] < 0) t = fe29_norm(fe29_add(t, pl));
  const Fe29<FP> s = fe29_norm(fe29_sub(t, pl));
  if (s.v[8] >= 0) t = s;
  return fe29_pack(t);
}

// A value in the API form (x 2^256, canonical) as a product operand without a conversion product: shifted left by five
// bits while it is unpacked it is the integer x 2^261 + (a multiple of p) < 32 p, the working form of x; minus 16 p it
// lies in (-16 p, 16 p) with limbs of magnitude < 2^29 (a valid operand of fe29_mul on either side).
template <class FP>
H2_HD Fe29<FP> expr_column_operand(const Fe<FP>& a) {
  Fe29<FP> r;
#pragma unroll
  for (int j = 0; j < 9; j++) {
    // limb j of (a << 5): bits [29 j - 5, 29 j + 24) of a
    const int bit = 29 * j - 5;
    uint32_t limb;
    if (bit < 0) {
      limb = (a.v[0] << 5) & L29_MASK;
    } else {
      const int w = bit >> 5, sh = bit & 31;
      const uint64_t lo = a.v[w], hi = w + 1 < 8 ? a.v[w + 1] : 0;
      limb = (uint32_t)((lo | (hi << 32)) >> sh) & L29_MASK;
    }
    // minus 16 p = (p << 4): limb j of it is bits [29 j - 4, 29 j + 25) of p
    const int pb = 29 * j - 4;
    uint32_t pl;
    if (pb < 0) {
      pl = (FP::P(0) << 4) & L29_MASK;
    } else {
      const int w = pb >> 5, sh = pb & 31;
      const uint64_t lo = w < 8 ? FP::P(w) : 0, hi = w + 1 < 8 ? FP::P(w + 1) : 0;
      pl = (uint32_t)((lo | (hi << 32)) >> sh) & L29_MASK;
    }
    r.v[j] = (int32_t)limb - (int32_t)pl;
  }
  return r;
}

// a^(p-2) on the working form, two exponent bits at a time (254 squarings + ~96 products); a normalised, of small
// magnitude (a product's result); the exponent is a constant, so the branches are uniform
template <class FP>
H2_HD Fe29<FP> fe29_inv(const Fe29<FP>& a) {
  const Fe29<FP> a2 = fe29_mul(a, a), a3 = fe29_mul(a2, a);
  uint32_t e[8];
  uint32_t borrow = 2;
#pragma unroll
  for (int i = 0; i < 8; i++) {               // p - 2, with the borrow of the Pasta primes (p[0] = 1)
    const uint32_t w = FP::P(i);
    e[i] = w - borrow;
    borrow = w < borrow ? 1u : 0u;
  }
  Fe29<FP> r = fe29_from_api(Fe<FP>::one());
  for (int i = 254; i >= 0; i -= 2) {
    r = fe29_mul(r, r);
    r = fe29_mul(r, r);
    const uint32_t d = (e[i >> 5] >> (i & 31)) & 3u;
    if (d == 1) r = fe29_mul(r, a);
    else if (d == 2) r = fe29_mul(r, a2);
    else if (d == 3) r = fe29_mul(r, a3);
  }
  return r;
}

// x == 0 mod p for a loosely reduced x (|x| < 16 p: the callers pass differences of a few products and normalised
// values, |x| < 4p): if x = j p then j = x[0] p^-1 mod 2^29 is in (-16, 16) -- anything else is rejected by that one
// limb; the rare survivors are reduced completely (fe29_to_api takes any |x| < 64 p)
template <class FP>
H2_HD bool fe29_is_zero_mod_p(const Fe29<FP>& a) {
  constexpr uint32_t pinv = (0u - (FP::INV & L29_MASK)) & L29_MASK;  // p^-1 mod 2^29
  const uint32_t j = ((uint32_t)a.v[0] * pinv) & L29_MASK;
  if (j > 16u && j < (1u << 29) - 16u) return false;
  return fe29_to_api(a).is_zero();
}

}  // namespace h2
