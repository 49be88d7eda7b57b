// h2_field29_chain.hpp -- the Montgomery product of h2_field29.hpp with ONE multiply-add chain per column, for the
// kernels in which several waves share a SIMD (msm_chunk_kernel: three, the NTT pass: four).
//
// Why: from `acc += a_i b_j` the optimiser builds two chains per column, the a b terms and the m p terms, and joins
// them with a 64-bit add; around the join it moves the carry between register pairs.  For a
// lone wave that is right -- a dependent v_mad_i64_i32 waits 12-13 cycles for its addend -- but with three or four
// waves per SIMD a wave's consecutive multiply-adds are 16-21 cycles apart anyway, and the join and its moves are issue
// slots that compute nothing.  Two rewordings of the C++ did not change what the optimiser builds.  Here the limb
// products are v_mad_i64_i32 instructions in asm statements, each with the accumulator it writes as its addend: the
// optimiser can neither reassociate the column nor choose another instruction, the carry of column K is the addend of
// column K + 1's first multiply-add, and what is left to the compiler per column is the AND that takes m (or the
// output limb) and the arithmetic shift that hands the column on.
//
// Why a statement per RUN of multiply-adds (a column's limb products; a column's m p terms) and not one block per
// product: a 64-bit accumulator is one "v" operand (a register pair), the AND needs its low word, and the AMDGPU
// inline assembler has no operand modifier that names half of a pair -- so the AND and the shift stay in C++ and a
// block ends where they come.  And not one statement per multiply-add: gfx950 has a forwarding hazard that the
// compiler cannot rule out for code it does not see, so it puts one wait state (s_nop 0) between an asm statement and a
// consumer of its result that follows directly; per multiply-add that was 143 per product, per run it is ~25, issued by
// the wave's scalar path while the SIMD serves another wave (profiles/fe29_chain_isa.txt).  The statements touch no
// memory and no scalar state: the carry-out pair that the VOP3B encoding writes goes to a dummy scalar output (a `vcc`
// clobber would order all the statements of a kernel among themselves).
//
// A paired form -- two independent products of the mixed addition interleaved multiply-add by multiply-add in the
// same statements -- was built and measured: within the unpaired form's run-to-run range, not kept
// (profiles/fe29_chain_parent_vs_branch.txt, section 4).
//
// Same integer operations modulo 2^64 as detail29::columns: m[K] = the low 29 bits of column K (p = 1 mod 2^29, the
// p[0] term is never computed), acc += m_i (-p[j]) for the non-zero limbs of p, an arithmetic shift by 29.  The nine
// output limbs are therefore IDENTICAL to fe29_mul's, fe29_sqr's, fe29_mul_sub's and fe29_mul_up's, not merely
// congruent (tests/test_gpu_fe29_chain.py); every bound in h2_field29.hpp, h2_curve29.hpp and h2_ntt29.hpp holds as
// written.  Device code only, and only for moduli with p = 1 mod 2^29 (the Pasta primes): Fe29Chain falls back to the
// compiler's form on the host and for BN254, whose dense modulus and quarter-rate m are another problem.
#pragma once
#include "h2_field29.hpp"
#include <utility>

namespace h2 {

namespace chain29 {
// p = 1 mod 2^29: m is the column's own low 29 bits
template <class FP>
constexpr bool covers() {
  return ((0u - (FP::INV & L29_MASK)) & L29_MASK) == 1u;
}
#if defined(__HIP_DEVICE_COMPILE__)
// acc = x y: the product's first multiply-add
__device__ __forceinline__ void mad_first(int64_t& acc, int32_t x, int32_t y) {
  uint64_t co;
  asm("v_mad_i64_i32 %0, %1, %2, %3, 0" : "=v"(acc), "=&s"(co) : "v"(x), "v"(y));
}
// Run<N, SC>::go: acc += x[0] y[0] + ... + x[N - 1] y[N - 1] as N multiply-adds in one statement (behind a statement
// the compiler fills the one wait state it cannot rule out for whatever reads the result next, so a run is one
// statement, not N).  SC: the y are limbs of -p (of p: the additive form) in scalar registers
template <int N, bool SC>
struct Run;
#define H2_CH_M(x, y) "v_mad_i64_i32 %0, %1, %" #x ", %" #y ", %0\n\t"
#define H2_CH_T1 H2_CH_M(2, 3)
#define H2_CH_T2 H2_CH_T1 H2_CH_M(4, 5)
#define H2_CH_T3 H2_CH_T2 H2_CH_M(6, 7)
#define H2_CH_T4 H2_CH_T3 H2_CH_M(8, 9)
#define H2_CH_T5 H2_CH_T4 H2_CH_M(10, 11)
#define H2_CH_T6 H2_CH_T5 H2_CH_M(12, 13)
#define H2_CH_T7 H2_CH_T6 H2_CH_M(14, 15)
#define H2_CH_T8 H2_CH_T7 H2_CH_M(16, 17)
#define H2_CH_T9 H2_CH_T8 H2_CH_M(18, 19)
#define H2_CH_IN1(C) "v"(x[0]), C(y[0])
#define H2_CH_IN2(C) H2_CH_IN1(C), "v"(x[1]), C(y[1])
#define H2_CH_IN3(C) H2_CH_IN2(C), "v"(x[2]), C(y[2])
#define H2_CH_IN4(C) H2_CH_IN3(C), "v"(x[3]), C(y[3])
#define H2_CH_IN5(C) H2_CH_IN4(C), "v"(x[4]), C(y[4])
#define H2_CH_IN6(C) H2_CH_IN5(C), "v"(x[5]), C(y[5])
#define H2_CH_IN7(C) H2_CH_IN6(C), "v"(x[6]), C(y[6])
#define H2_CH_IN8(C) H2_CH_IN7(C), "v"(x[7]), C(y[7])
#define H2_CH_IN9(C) H2_CH_IN8(C), "v"(x[8]), C(y[8])
#define H2_CH_RUN(N)                                                                                  \
  template <>                                                                                         \
  struct Run<N, false> {                                                                              \
    static __device__ __forceinline__ void go(int64_t& acc, const int32_t* x, const int32_t* y) {     \
      uint64_t co;                                                                                    \
      asm(H2_CH_T##N : "+v"(acc), "=&s"(co) : H2_CH_IN##N("v"));                                      \
    }                                                                                                 \
  };                                                                                                  \
  template <>                                                                                         \
  struct Run<N, true> {                                                                               \
    static __device__ __forceinline__ void go(int64_t& acc, const int32_t* x, const int32_t* y) {     \
      uint64_t co;                                                                                    \
      asm(H2_CH_T##N : "+v"(acc), "=&s"(co) : H2_CH_IN##N("s"));                                      \
    }                                                                                                 \
  };
H2_CH_RUN(1) H2_CH_RUN(2) H2_CH_RUN(3) H2_CH_RUN(4) H2_CH_RUN(5) H2_CH_RUN(6) H2_CH_RUN(7) H2_CH_RUN(8) H2_CH_RUN(9)
#undef H2_CH_RUN
#undef H2_CH_M
#undef H2_CH_T1
#undef H2_CH_T2
#undef H2_CH_T3
#undef H2_CH_T4
#undef H2_CH_T5
#undef H2_CH_T6
#undef H2_CH_T7
#undef H2_CH_T8
#undef H2_CH_T9
#undef H2_CH_IN1
#undef H2_CH_IN2
#undef H2_CH_IN3
#undef H2_CH_IN4
#undef H2_CH_IN5
#undef H2_CH_IN6
#undef H2_CH_IN7
#undef H2_CH_IN8
#undef H2_CH_IN9
template <>
struct Run<0, true> {
  static __device__ __forceinline__ void go(int64_t&, const int32_t*, const int32_t*) {}
};

// the limb products a[I] b[K - I], I = LO + Ns, of column K (the product's very first one sets the accumulator)
template <int K, int LO, bool FIRST, int... Ns>
__device__ __forceinline__ void col_ab(int64_t& acc, const int32_t* a, const int32_t* b, std::integer_sequence<int, Ns...>) {
  if constexpr (FIRST) {
    static_assert(K == 0 && sizeof...(Ns) == 1, "column 0 is one product");
    mad_first(acc, a[0], b[0]);
  } else {
    const int32_t x[] = {a[LO + Ns]...}, y[] = {b[K - LO - Ns]...};
    Run<(int)sizeof...(Ns), false>::go(acc, x, y);
  }
}
// column K of a^2: cross terms against the doubled operand, the square of the middle limb once
template <int K, int LO, bool FIRST, int... Ns>
__device__ __forceinline__ void col_sq(int64_t& acc, const int32_t* a, const int32_t* a2, std::integer_sequence<int, Ns...>) {
  if constexpr (FIRST) {
    static_assert(K == 0 && sizeof...(Ns) == 1, "column 0 is one product");
    mad_first(acc, a[0], a[0]);
  } else {
    const int32_t x[] = {a[LO + Ns]...}, y[] = {(LO + Ns < K - LO - Ns ? a2[K - LO - Ns] : a[LO + Ns])...};
    Run<(int)sizeof...(Ns), false>::go(acc, x, y);
  }
}
// the m p terms m[I] p[K - I], LO <= I <= HI, of column K: the zero limbs of p cost nothing
template <class FP>
constexpr int mp_count(int K, int LO, int HI) {
  int n = 0;
  for (int i = LO; i <= HI; i++) n += fe29_p<FP>(K - i) != 0 ? 1 : 0;
  return n;
}
template <class FP>
constexpr int mp_index(int K, int LO, int HI, int nth) {   // the I of the nth non-zero term
  for (int i = LO; i <= HI; i++)
    if (fe29_p<FP>(K - i) != 0 && nth-- == 0) return i;
  return LO;
}
template <class FP, int K, int LO, int HI, bool UP, int... Ns>
__device__ __forceinline__ void col_mp(int64_t& acc, const int32_t* m, std::integer_sequence<int, Ns...>) {
  if constexpr (sizeof...(Ns) != 0) {
    const int32_t x[] = {m[mp_index<FP>(K, LO, HI, Ns)]...};
    const int32_t y[] = {(UP ? (int32_t)fe29_p<FP>(K - mp_index<FP>(K, LO, HI, Ns))
                             : -(int32_t)fe29_p<FP>(K - mp_index<FP>(K, LO, HI, Ns)))...};
    Run<(int)sizeof...(Ns), true>::go(acc, x, y);
  }
}
// after column K's limb products: its m p terms, m[K] or output limb K - 9, the hand-over.  UP (fe29_mul_up): m is
// the NEGATED low 29 bits and m p is added, p[0] = 1 included (its term clears the bits the shift drops exactly)
template <class FP, int K, bool UP>
__device__ __forceinline__ void reduce_col(int64_t& acc, int32_t* m, int32_t* t) {
  constexpr int LO = K < 9 ? 0 : K - 8, HI = K < 9 ? K - 1 : 8;
  col_mp<FP, K, LO, HI, UP>(acc, m, std::make_integer_sequence<int, mp_count<FP>(K, LO, HI)>{});
  if constexpr (K < 9) {
    if constexpr (UP) {
      m[K] = (int32_t)((0u - (uint32_t)acc) & L29_MASK);
      const int32_t one = 1;
      Run<1, true>::go(acc, &m[K], &one);
    } else {
      m[K] = (int32_t)((uint32_t)acc & L29_MASK);
    }
  } else {
    t[K - 9] = (int32_t)((uint32_t)acc & L29_MASK);
  }
  acc >>= 29;
}
template <class FP, int K, bool UP>
__device__ __forceinline__ void columns(int64_t& acc, const int32_t* a, const int32_t* b, int32_t* m, int32_t* t) {
  if constexpr (K < 17) {
    constexpr int LO = K < 9 ? 0 : K - 8, HI = K < 9 ? K : 8;
    col_ab<K, LO, K == 0>(acc, a, b, std::make_integer_sequence<int, HI - LO + 1>{});
    reduce_col<FP, K, UP>(acc, m, t);
    columns<FP, K + 1, UP>(acc, a, b, m, t);
  }
}
template <class FP, int K>
__device__ __forceinline__ void columns_sq(int64_t& acc, const int32_t* a, const int32_t* a2, int32_t* m, int32_t* t) {
  if constexpr (K < 17) {
    constexpr int LO = K < 9 ? 0 : K - 8, HI = K / 2;
    col_sq<K, LO, K == 0>(acc, a, a2, std::make_integer_sequence<int, HI - LO + 1>{});
    reduce_col<FP, K, false>(acc, m, t);
    columns_sq<FP, K + 1>(acc, a, a2, m, t);
  }
}
template <class FP, int K>
__device__ __forceinline__ void columns2(int64_t& acc, const int32_t* a, const int32_t* b, const int32_t* c, const int32_t* d,
                                         int32_t* m, int32_t* t) {
  if constexpr (K < 17) {
    constexpr int LO = K < 9 ? 0 : K - 8, HI = K < 9 ? K : 8;
    col_ab<K, LO, K == 0>(acc, a, b, std::make_integer_sequence<int, HI - LO + 1>{});
    col_ab<K, LO, false>(acc, c, d, std::make_integer_sequence<int, HI - LO + 1>{});
    reduce_col<FP, K, false>(acc, m, t);
    columns2<FP, K + 1>(acc, a, b, c, d, m, t);
  }
}

// fe29_mul (UP: fe29_mul_up), the same limbs
template <class FP, bool UP>
__device__ __forceinline__ Fe29<FP> mul(const Fe29<FP>& a, const Fe29<FP>& b) {
  int64_t acc;
  int32_t m[9];
  Fe29<FP> r;
  columns<FP, 0, UP>(acc, a.v, b.v, m, r.v);
  r.v[8] = (int32_t)acc;
  return r;
}
// fe29_sqr, the same limbs
template <class FP>
__device__ __forceinline__ Fe29<FP> sqr(const Fe29<FP>& a) {
  int64_t acc;
  int32_t m[9], a2[9];
#pragma unroll
  for (int i = 0; i < 9; i++) a2[i] = a.v[i] * 2;
  Fe29<FP> r;
  columns_sq<FP, 0>(acc, a.v, a2, m, r.v);
  r.v[8] = (int32_t)acc;
  return r;
}
// fe29_mul_sub, the same limbs
template <class FP>
__device__ __forceinline__ Fe29<FP> mul_sub(const Fe29<FP>& a, const Fe29<FP>& b, const Fe29<FP>& c, const Fe29<FP>& d) {
  int64_t acc;
  int32_t m[9], nc[9];
#pragma unroll
  for (int i = 0; i < 9; i++) nc[i] = -c.v[i];
  Fe29<FP> r;
  columns2<FP, 0>(acc, a.v, b.v, nc, d.v, m, r.v);
  r.v[8] = (int32_t)acc;
  return r;
}
#endif  // __HIP_DEVICE_COMPILE__
}  // namespace chain29

// The arithmetic policies of the templates that take one (xyzz29_add_affine, the NTT pass body): which form of the
// product a kernel's instantiation is built from.  Fe29Compiler is h2_field29.hpp as every other caller sees it.
struct Fe29Compiler {
  template <class FP> static H2_HD Fe29<FP> mul(const Fe29<FP>& a, const Fe29<FP>& b) { return fe29_mul(a, b); }
  template <class FP> static H2_HD Fe29<FP> mul_up(const Fe29<FP>& a, const Fe29<FP>& b) { return fe29_mul_up(a, b); }
  template <class FP> static H2_HD Fe29<FP> sqr(const Fe29<FP>& a) { return fe29_sqr(a); }
  template <class FP>
  static H2_HD Fe29<FP> mul_sub(const Fe29<FP>& a, const Fe29<FP>& b, const Fe29<FP>& c, const Fe29<FP>& d) {
    return fe29_mul_sub(a, b, c, d);
  }
};
// The chain forms where they exist (device code, p = 1 mod 2^29), the compiler's form everywhere else
struct Fe29Chain {
  template <class FP> static H2_HD Fe29<FP> mul(const Fe29<FP>& a, const Fe29<FP>& b) {
#if defined(__HIP_DEVICE_COMPILE__)
    if constexpr (chain29::covers<FP>()) return chain29::mul<FP, false>(a, b);
#endif
    return fe29_mul(a, b);
  }
  template <class FP> static H2_HD Fe29<FP> mul_up(const Fe29<FP>& a, const Fe29<FP>& b) {
#if defined(__HIP_DEVICE_COMPILE__)
    if constexpr (chain29::covers<FP>()) return chain29::mul<FP, true>(a, b);
#endif
    return fe29_mul_up(a, b);
  }
  template <class FP> static H2_HD Fe29<FP> sqr(const Fe29<FP>& a) {
#if defined(__HIP_DEVICE_COMPILE__)
    if constexpr (chain29::covers<FP>()) return chain29::sqr(a);
#endif
    return fe29_sqr(a);
  }
  template <class FP>
  static H2_HD Fe29<FP> mul_sub(const Fe29<FP>& a, const Fe29<FP>& b, const Fe29<FP>& c, const Fe29<FP>& d) {
#if defined(__HIP_DEVICE_COMPILE__)
    if constexpr (chain29::covers<FP>()) return chain29::mul_sub(a, b, c, d);
#endif
    return fe29_mul_sub(a, b, c, d);
  }
};

}  // namespace h2
