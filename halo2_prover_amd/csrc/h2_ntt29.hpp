// h2_ntt29.hpp -- the NTT pass kernel: butterflies on the 9 x 29-bit lazy form (h2_field29.hpp).
//
// Device replacement for halo2_proofs::arithmetic::best_fft / recursive_butterfly_arithmetic (plan and contract in
// h2_ntt.hpp).  HBM keeps the API's format (4 x u64 Montgomery limbs, R = 2^256); between the tile load and the tile
// store everything is on the working form:
//   * x 2^256 mod p (the API's bytes) is the R' = 2^261 form of x / 32, and the transform is linear: the DATA need no
//     conversion at all, only the twiddle tables are built in R' form;
//   * a product costs 81 + 9k multiply-adds without carry counters or a conditional subtraction, additions and
//     subtractions are nine limb operations without carries; every value written back to LDS is carry-normalised
//     (limbs in [0, 2^29), the top limb takes the sign);
//   * magnitudes: a tile's inputs are below 3p/2 IN MAGNITUDE.  The plain pass reads values in [0, 3p/2): canonical
//     API data, or what a non-final pass stored (see below).  The EXTENDING pass 0 (EvaluationDomain::coeff_to_extended,
//     at the end of this comment) reads canonical data in [0, p) and multiplies two of every three elements by zeta or
//     zeta^2 on the way in: fe29_mul of two canonical operands (|a| |b| < p^2, far inside 64 p^2) is in
//     (a b / R' - p, a b / R'], i.e. in (-p, p/128] -- inside the product's general (-3p/2, p/2], normalised, the top
//     limb signed like every value the stages keep in LDS; an element beyond the source's length is exact zero.  The
//     DIVIDING pass 0 (EvaluationDomain::divide_by_vanishing_poly on the way into extended_to_coeff, at the end of
//     this comment) is the same case with another constant: canonical data times a canonical t[i mod period], in
//     (-p, p/128], on EVERY element.  So
//     there a tile input lies in (-3p/2, p/2) or [0, p), not in [0, 3p/2): the sign differs, the magnitude does not,
//     and nothing below uses the sign.  A radix-4 double stage adds at most two products (each in (-3p/2, p/2)) to an
//     element, the very first one (all twiddles 1) at most quadruples it: |x| <= 4 * 1.5p + 3p * 4 = 18p after the
//     five double stages of a 1024-row tile, well inside fe29_mul's |a| |b| <= 64 p^2 with a canonical twiddle as b.
//     The first stage's operands are sums and differences of two inputs: normalised limbs 0..7 in [0, 2^29) and a
//     top limb of magnitude below 2^24 whatever the sign, so their limbs stay within +-2^29 as fe29_mul asks.  The
//     exits take either sign: a non-final pass adds 32p first, the final one indexes the canonicalisation table by
//     the SIGNED top limb (|t| <= 144 < NTT_CANON_OFF).
// Round 3: what the pass did besides products:
//   * leaving a NON-FINAL pass an element x is multiplied by the inter-pass twiddle anyway.  It is first moved to
//     32p + x (or 32p - x where the exponent asks for -w: the negation costs nothing) -- positive, limbs below 2^30 --
//     so the product rounded up (fe29_mul_up) lies in [0, 1.5p) and its limbs pack to 256 bits as they are: no carry
//     pass, no conditional additions.  The stored value is a representative below 2^256, not the canonical one; only
//     the next pass reads it;
//   * leaving the FINAL pass nothing is multiplied (round 2: a 240-instruction product with 1 on every element of every
//     forward transform): t = floor(x / 2^252) is read off the top limb and x - T[t] with T[t] = floor(t 2^252 / p) p
//     from a 300-entry table lies in [0, p + 2^252): one conditional subtraction makes it canonical;
//   * a transform scaled by a constant (EvaluationDomain::ifft's 1/n) in two passes uses inter-pass twiddles that carry
//     the constant (table built once per (omega, log n, constant)): no product in its final pass either;
//   * the radix twiddles are kept UNPACKED (36 bytes in three planes, in LDS or -- 1024-row tiles -- global memory):
//     three loads per use instead of two loads and a 27-instruction unpack, three times per radix-4 group.
// The extending pass 0 (ntt29_extend_pass_kernel, the template flag EXT of the pass body; h2_coeff_to_extended_device):
//   coeff_to_extended is "pad the n coefficients with zeros to 2^ext_k, multiply element i by zeta^i, transform".  As
//   two launches that writes a column that is mostly zeros and reads it back.  Pass 0 loads its tile straight from HBM
//   into registers, so the padding and the factor ride on that load: the source is a separate, read-only buffer of
//   columns of n elements (any stride >= n); a tile element whose SOURCE INDEX -- i_first + cc + (j << log_inner) in a
//   non-final pass 0 (log_outer = 0: the tile's in_base is i_first), j in a one-pass plan -- is >= n is zero and is not
//   loaded; a loaded one with index = 1, 2 mod 3 is multiplied by zeta, zeta^2 (zeta^3 = 1: at most 2n/3 products per
//   column, the only extra arithmetic).  Everything behind the load is the plain pass; later passes ARE the plain
//   kernel.  The plain kernel is its own instantiation (EXT = false): same registers and occupancy as before the flag
//   existed (profiles/coeff_to_extended_resources.txt).  The butterflies on known zeros are NOT skipped (with 2^e-fold
//   padding the first e stages are copies times twiddles): not built, not measured.
// The dividing pass 0 and the shrinking final pass (the template flags DIV and SHR; h2_extended_to_coeff_device):
//   extended_to_coeff is "transform with ext_omega^-1, times 1 / 2^ext_k, times zeta^-j, keep the first n (d - 1)
//   coefficients", and the prover divides by the vanishing polynomial (element i times t[i mod period]) just before.
//   Composed, that is two more passes over the whole extended column and a copy of its kept prefix.  Here:
//   * DIV, pass 0: load_el multiplies element i -- the same index as EXT's -- by t[i mod period].  t comes in the API
//     form and the product needs the R' form: five doublings per table ENTRY, done once per block into LDS behind the
//     tile where the block needs at most NTT_DIV_LDS_MAX entries (any period up to 2^log_inner: one entry per tile
//     column), at the element's load otherwise (then an entry serves fewer than RC / NTT_DIV_LDS_MAX elements of the
//     block; with period = 2^log_n, exactly one).  The staging is followed by a barrier of its own: the fused first
//     stage loads before the block's first barrier;
//   * SHR, the final pass: emit knows its output index out_base + (k << out_k_shift) + cc.  At or beyond out_len it
//     returns before any arithmetic -- k holds the index's top bits, so with out_len <= 3/4 2^log_n a quarter of the
//     last radix-4 stage's register outputs leave without a product, a canonicalisation or a store.  Otherwise the
//     index mod 3 picks the exit: with has_scale (one and three passes) the scale's product takes scale, scale zeta^-1
//     or scale zeta^-2 -- the un-shift costs nothing; in a two-pass plan (the scale rides in the inter-pass twiddles,
//     the table h2_ntt_scaled_device uses) index = 0 mod 3 takes the product-free canonicalisation and the other two
//     one product by zeta^-1 or zeta^-2 through the same positive-operand path (32p + x times a canonical constant,
//     rounded up, minus p: in [-p, 50p/128), canonical after at most one addition).  The destination's columns are
//     out_stride apart and nothing is written at or beyond out_len;
//   * a one-pass plan (log n <= 10) is both at once; without a t table pass 0 of a longer plan is the plain kernel.
//   The plain and the extending instantiations do not depend on anything that is `if constexpr (DIV)` or `(SHR)`: same
//   registers and occupancy as before the flags existed (profiles/extended_to_coeff_resources.txt).
// LDS: 36 bytes per element in three planes (two of 16 bytes, one of 4: ds_read_b128 x 2 + ds_read_b32).
#pragma once
#include "h2_field29_chain.hpp"
#include "h2_ntt.hpp"
#include <algorithm>

namespace h2 {

// ---- tables ----------------------------------------------------------------------------------------------------------
// One allocation per (field, omega, log n, constant):
//   main   [n/2] x 32 B   first * omega^i in R' form, canonical, packed (the inter-pass twiddles; first = 1 or the constant)
//   radix  per pass: [R/2] unpacked twiddles omega^(i n / R) in three planes (16 B, 16 B, 4 B)
//   canon  [NTT_CANON_N] multiples of p, unpacked, one 36-byte row each: T[t + NTT_CANON_OFF] = floor(t 2^252 / p) p
constexpr int NTT_CANON_OFF = 192, NTT_CANON_N = 384;   // |x| <= 18p < 18 * 2^255: |t| = |x| / 2^252 <= 144
struct NttTables {
  size_t off_radix[3], off_canon, total;                // bytes from the start of the allocation
};
inline NttTables ntt29_tables(uint32_t log_n) {
  NttTables t{};
  const NttPlan pl = ntt_make_plan(log_n);
  size_t o = (((size_t)1 << log_n) / 2) * 32;
  if (o < 64) o = 64;
  for (int p = 0; p < 3; p++) {
    t.off_radix[p] = o;
    if (p < pl.npass) o += ((((size_t)1 << pl.pass[p].log_r) / 2) * 36 + 255) & ~(size_t)255;
  }
  t.off_canon = o;
  o += (size_t)NTT_CANON_N * 36;
  t.total = (o + 255) & ~(size_t)255;
  return t;
}

// main[i] = first * omega^i (R' form, canonical, packed) for i < half_n
template <class FP>
__global__ void __launch_bounds__(256) ntt_twiddle29_kernel(U128* tw, Fe<FP> omega, Fe<FP> first, uint32_t half_n) {
  uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  uint64_t start = (uint64_t)t * TW_RUN;
  if (start >= half_n) return;
  Fe<FP> cur = fe_mul(first, fe_pow_u64(omega, start));
  for (int k = 0; k < TW_RUN && start + k < half_n; k++) {
    Fe<FP> r = cur;
#pragma unroll
    for (int d = 0; d < 5; d++) r = fe_dbl(r);            // x 2^256 -> x 2^261
    fe_store<FP>(tw + 2 * (start + k), r);
    cur = fe_mul(cur, omega);
  }
}
// radix[i] = omega^(i << shift), unpacked, planes of `half_r` entries: limbs 0..3 | limbs 4..7 | limb 8
template <class FP>
__global__ void __launch_bounds__(256) ntt_radix29_kernel(uint32_t* radix, Fe<FP> omega, uint32_t half_r, uint32_t shift) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= half_r) return;
  Fe<FP> r = fe_pow_u64(omega, (uint64_t)i << shift);
#pragma unroll
  for (int d = 0; d < 5; d++) r = fe_dbl(r);
  const Fe29<FP> u = fe29_unpack(r);
  uint32_t* p0 = radix + 4 * (size_t)i;
  uint32_t* p1 = radix + 4 * (size_t)half_r + 4 * (size_t)i;
  uint32_t* p2 = radix + 8 * (size_t)half_r + i;
#pragma unroll
  for (int l = 0; l < 4; l++) {
    p0[l] = (uint32_t)u.v[l];
    p1[l] = (uint32_t)u.v[4 + l];
  }
  p2[0] = (uint32_t)u.v[8];
}
// canon[t + OFF] = floor(t 2^252 / p) * p as nine normalised limbs (the top one signed): thread t finds the quotient q
// with 0 <= t 2^252 - q p < p by exact limb arithmetic starting from a floating-point estimate
template <class FP>
__global__ void __launch_bounds__(64) ntt_canon29_kernel(int32_t* canon) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= NTT_CANON_N) return;
  const int t = idx - NTT_CANON_OFF;
  double pd = 0;                                          // p / 2^232
  for (int j = 0; j < 9; j++) pd += (double)fe29_p<FP>(j) * exp2((double)(29 * j - 232));
  int q = (int)floor((double)t * 1048576.0 / pd);        // t 2^252 / p = t 2^20 / (p / 2^232)
  int64_t d[9];
  for (int tries = 0; tries < 8; tries++) {
    // d = t 2^252 - q p, carry-normalised (top limb signed)
    int64_t carry = 0;
    for (int j = 0; j < 9; j++) {
      int64_t v = -(int64_t)q * (int64_t)fe29_p<FP>(j) + carry + (j == 8 ? (int64_t)t * 1048576 : 0);
      if (j < 8) {
        d[j] = v & L29_MASK;
        carry = v >> 29;
      } else {
        d[j] = v;
      }
    }
    if (d[8] < 0) { q--; continue; }
    // d >= p ?
    int64_t borrow = 0;
    for (int j = 0; j < 9; j++) {
      const int64_t v = d[j] - (int64_t)fe29_p<FP>(j) + borrow;
      borrow = j < 8 ? (v >> 29) : v;                    // after the last limb: the sign of d - p
    }
    if (borrow >= 0) { q++; continue; }
    break;
  }
  // the row: q p, normalised
  int64_t carry = 0;
  for (int j = 0; j < 9; j++) {
    const int64_t v = (int64_t)q * (int64_t)fe29_p<FP>(j) + carry;
    if (j < 8) {
      canon[9 * idx + j] = (int32_t)(v & L29_MASK);
      carry = v >> 29;
    } else {
      canon[9 * idx + j] = (int32_t)v;
    }
  }
}

// What the EXTENDING pass 0 takes besides the plain pass's arguments (EvaluationDomain::coeff_to_extended in one call,
// ntt29_extend_launch): the source is another buffer of shorter columns, zero beyond them, times zeta^i on the way in.
template <class FP>
struct NttExtend {
  size_t src_stride;   // elements between the source's columns
  uint32_t n;          // the source's length: a tile element whose source index is >= n is zero and is not loaded
  Fe<FP> z1, z2;       // zeta and zeta^2 (zeta^3 = 1), R' form, canonical
};

// What the DIVIDING pass 0 and the SHRINKING final pass take besides the plain pass's arguments
// (EvaluationDomain::extended_to_coeff in one call, ntt29_coeff_launch; a one-pass plan uses both halves).
constexpr uint32_t NTT_DIV_LDS_MAX = 128;   // converted t entries a block keeps in LDS (32 B each: 4 KB at most)
template <class FP>
struct NttCoeff {
  // DIV: element i of a column is multiplied by t[i & t_mask] on its way into pass 0
  const U128* t;        // t_mask + 1 canonical elements, API form
  uint32_t t_mask;
  uint32_t t_jbits;     // how many low bits of the tile row j reach the index's bits below the period (0: only cc does)
  uint32_t t_staged;    // the block's (C << t_jbits) entries are converted once, into LDS at t_lds_off
  uint32_t t_lds_off;   // in 16-byte units from the start of dynamic LDS (behind everything the plain pass uses)
  // SHR: the final pass stores out[c][j] for j < out_len only, columns out_stride apart, times c[j mod 3]
  uint32_t out_len;
  size_t out_stride;
  Fe<FP> c0, c1, c2;    // R' form, canonical.  has_scale: scale, scale zeta^-1, scale zeta^-2; else c0 unused, zeta^-1, zeta^-2
};

// The pass.  EXT = DIV = SHR = false is the transform as it always was (ntt29_pass_kernel: its code does not depend on
// anything below that is `if constexpr` of a flag); EXT is pass 0 of an extending transform
// (ntt29_extend_pass_kernel); DIV is pass 0 and SHR the final pass of extended_to_coeff (ntt29_coeff_pass_kernel).
template <class FP, bool EXT, bool DIV = false, bool SHR = false>
__device__ __forceinline__ void
ntt29_pass_body(const U128* __restrict__ in, U128* __restrict__ out, const U128* __restrict__ tw,
                const uint32_t* __restrict__ radix /* this pass's unpacked radix twiddles */,
                const int32_t* __restrict__ canon, const NttPass& P, size_t col_stride /* elements */,
                const Fe<FP>& scale29 /* R' form, canonical; used when P.has_scale */, const NttExtend<FP>* X,
                const NttCoeff<FP>* Y = nullptr) {
  static_assert(!(EXT && (DIV || SHR)), "the extending pass 0 neither divides nor shrinks");
  // the products of radix4, emit and load_el: the single-chain form where it exists (the Pasta fields; four waves per
  // SIMD cover its latency), the compiler's for BN254 -- the same limbs either way (h2_field29_chain.hpp)
  using AR = Fe29Chain;
  extern __shared__ U128 lds[];
  const uint32_t R = 1u << P.log_r, C = 1u << P.log_c;
  const uint32_t RC = R * C;
  const uint32_t n_half_log = P.log_n - 1;
  U128* tile0 = lds;                                   // limbs 0..3
  U128* tile1 = lds + RC;                              // limbs 4..7
  int32_t* tile2 = reinterpret_cast<int32_t*>(lds + 2 * RC);     // limb 8
  U128* twl0 = lds + 2 * RC + ((RC + 3) >> 2);         // radix twiddles, unpacked, three planes (absent when P.tw_global)
  U128* twl1 = twl0 + (R >> 1);
  uint32_t* twl2 = reinterpret_cast<uint32_t*>(twl1 + (R >> 1));

  const U128* src = in + 2 * col_stride * blockIdx.y;
  U128* dst = out + 2 * col_stride * blockIdx.y;
  const uint32_t tid = threadIdx.x, nthr = blockDim.x;
  const uint32_t tile = blockIdx.x;

  // every stride is a power of two: addresses are shifts and adds (as 64-bit products they were 55 quarter-rate
  // multiplies per element in the write-back loop alone)
  uint64_t in_base, out_base;
  uint32_t in_j_shift, in_c_shift, out_k_shift;
  uint32_t i_first = 0;
  if (!P.is_final) {
    const uint32_t chunks = 1u << (P.log_inner - P.log_c);
    const uint32_t ic = tile & (chunks - 1), o = tile >> (P.log_inner - P.log_c);
    i_first = ic << P.log_c;
    in_base = ((uint64_t)o << (P.log_r + P.log_inner)) + i_first;
    in_j_shift = P.log_inner;
    in_c_shift = 0;
    out_base = in_base; out_k_shift = in_j_shift;
  } else {
    const uint32_t groups_log = P.log_r1 - P.log_c;
    const uint32_t k1c = tile & ((1u << groups_log) - 1), k2 = tile >> groups_log;
    const uint32_t k1 = k1c << P.log_c;
    in_base = (((uint64_t)k1 << P.log_r2) + k2) << P.log_r;
    in_j_shift = 0;
    in_c_shift = P.log_r2 + P.log_r;
    out_base = (uint64_t)k1 + ((uint64_t)k2 << P.log_r1);
    out_k_shift = P.log_r1 + P.log_r2;
  }
  src += 2 * in_base;
  if constexpr (SHR) dst = out + 2 * Y->out_stride * blockIdx.y;        // the kept prefixes, out_stride apart
  dst += 2 * out_base;
  [[maybe_unused]] const U128* xsrc = nullptr;          // EXT: this block's source column (read only through load_el)
  if constexpr (EXT) xsrc = in + 2 * X->src_stride * blockIdx.y;
  // DIV: entry ((jl << log_c) + cc) of the block's table is t[(i_first + cc + (jl << log_inner)) & t_mask] in R' form,
  // jl = the low t_jbits bits of the tile row (pass 0: log_outer = 0; a one-pass plan: log_inner = log_c = 0, i = j)
  [[maybe_unused]] U128* tlds = nullptr;
  if constexpr (DIV) {
    if (Y->t_staged) {
      tlds = lds + Y->t_lds_off;
      for (uint32_t li = tid; li < (C << Y->t_jbits); li += nthr) {
        const uint32_t ti = (i_first + (li & (C - 1)) + ((li >> P.log_c) << P.log_inner)) & Y->t_mask;
        Fe<FP> t = fe_load<FP>(Y->t + 2 * (size_t)ti);
#pragma unroll
        for (int d = 0; d < 5; d++) t = fe_dbl(t);       // x 2^256 -> x 2^261
        fe_store<FP>(tlds + 2 * li, t);
      }
      __syncthreads();                                   // (uniform: a kernel argument) the fused first stage loads next
    }
  }

  auto lds_put = [&](uint32_t i, const Fe29<FP>& u) {
    tile0[i] = U128{(uint32_t)u.v[0], (uint32_t)u.v[1], (uint32_t)u.v[2], (uint32_t)u.v[3]};
    tile1[i] = U128{(uint32_t)u.v[4], (uint32_t)u.v[5], (uint32_t)u.v[6], (uint32_t)u.v[7]};
    tile2[i] = u.v[8];
  };
  auto lds_get = [&](uint32_t i) {
    const U128 a0 = tile0[i], a1 = tile1[i];
    Fe29<FP> x;
    x.v[0] = (int32_t)a0.x; x.v[1] = (int32_t)a0.y; x.v[2] = (int32_t)a0.z; x.v[3] = (int32_t)a0.w;
    x.v[4] = (int32_t)a1.x; x.v[5] = (int32_t)a1.y; x.v[6] = (int32_t)a1.z; x.v[7] = (int32_t)a1.w;
    x.v[8] = tile2[i];
    return x;
  };
  const U128* rg0 = reinterpret_cast<const U128*>(radix);
  const U128* rg1 = rg0 + (R >> 1);
  const uint32_t* rg2 = radix + 8 * (size_t)(R >> 1);
  auto tw_get = [&](uint32_t i, bool from_table = false) {
    U128 t0, t1;
    Fe29<FP> t;
    if (P.tw_global || from_table) {
      t0 = rg0[i]; t1 = rg1[i];
      t.v[8] = (int32_t)rg2[i];
    } else {
      t0 = twl0[i]; t1 = twl1[i];
      t.v[8] = (int32_t)twl2[i];
    }
    t.v[0] = (int32_t)t0.x; t.v[1] = (int32_t)t0.y; t.v[2] = (int32_t)t0.z; t.v[3] = (int32_t)t0.w;
    t.v[4] = (int32_t)t1.x; t.v[5] = (int32_t)t1.y; t.v[6] = (int32_t)t1.z; t.v[7] = (int32_t)t1.w;
    return t;
  };

  // radix twiddles w_R^i = w^(i * n/R), i < R/2 (R' form, unpacked)
  if (!P.tw_global)
    for (uint32_t i = tid; i < (R >> 1); i += nthr) {
      twl0[i] = rg0[i];
      twl1[i] = rg1[i];
      twl2[i] = rg2[i];
    }
  // ---- leaving the tile: element k of column cc of the tile, carry-normalised ------------------------------------------
  Fe29<FP> pl, p32;                                     // p and 32 p as limbs (32 p: the limbs of p shifted five bits up)
#pragma unroll
  for (int i = 0; i < 9; i++) pl.v[i] = (int32_t)fe29_p<FP>(i);
  {
    int64_t carry = 0;
#pragma unroll
    for (int i = 0; i < 9; i++) {
      const int64_t v = ((int64_t)fe29_p<FP>(i) << 5) + carry;
      p32.v[i] = i < 8 ? (int32_t)(v & L29_MASK) : (int32_t)v;
      carry = v >> 29;
    }
  }
  auto emit = [&](uint32_t k, uint32_t cc, Fe29<FP> x) {
    Fe<FP> r;
    // SHR (always the final pass): nothing at all for an output at or beyond out_len; the others leave times
    // c[index mod 3] -- folded into the scale's product, or (no has_scale) a product only where index mod 3 != 0
    [[maybe_unused]] uint32_t r3 = 0;
    bool product = !P.is_final || P.has_scale;
    if constexpr (SHR) {
      const uint32_t oi = (uint32_t)out_base + (k << out_k_shift) + cc;      // < 2^log_n <= 2^30
      if (oi >= Y->out_len) return;
      r3 = oi % 3;
      product = P.has_scale || r3 != 0;
    }
    if (product) {
      // one product: the inter-pass twiddle w^(outer * i * k) (the table's entry 0 is 1, or the constant of a scaled
      // transform) or the final pass's scale.  32p +- x is positive (|x| <= 18p) with limbs below 2^30, so the product
      // rounded up (fe29_mul_up) is in [0, 50 p / 128 + p) and its limbs are those of a non-negative integer below
      // 2^256: packed as they are
      Fe29<FP> t;
      bool negate = false;
      if (!P.is_final) {
        const uint32_t ex = ((i_first + cc) * k) << P.log_outer;            // < n <= 2^30
        const uint32_t half_n = 1u << n_half_log;
        negate = ex >= half_n;
        t = fe29_unpack(fe_load<FP>(tw + 2 * (size_t)(negate ? ex - half_n : ex)));
      } else {
        if constexpr (SHR) t = fe29_unpack(r3 == 0 ? Y->c0 : (r3 == 1 ? Y->c1 : Y->c2));
        else t = fe29_unpack(scale29);
      }
      x = negate ? fe29_sub(p32, x) : fe29_add(p32, x);
      x = AR::mul_up(x, t);
      if (P.is_final) r = fe29_canonical_pack(fe29_norm(fe29_sub(x, pl)));   // a scaled final pass: canonical bytes
      else r = fe29_pack(x);
    } else {
      // no product: t = floor(x / 2^252) from the top limb (x is carry-normalised), x - T[t] in [0, p + 2^252)
      int32_t t = (x.v[8] >> 20) + NTT_CANON_OFF;
      t = t < 0 ? 0 : (t >= NTT_CANON_N ? NTT_CANON_N - 1 : t);       // (never: |x| <= 18p)
      const int32_t* row = canon + 9 * t;
      Fe29<FP> y;
#pragma unroll
      for (int i = 0; i < 9; i++) y.v[i] = x.v[i] - row[i];
      y = fe29_norm(y);
      const Fe29<FP> z = fe29_norm(fe29_sub(y, pl));
      r = fe29_pack(z.v[8] >= 0 ? z : y);
    }
    U128* g = dst + 2 * (((size_t)k << out_k_shift) + cc);
    g[0] = U128{r.v[0], r.v[1], r.v[2], r.v[3]};
    g[1] = U128{r.v[4], r.v[5], r.v[6], r.v[7]};
  };
  // element j of column cc of the tile, as the API's bytes (x 2^256 = the R' form of x / 32): one of the two shifts is 0
  // EXT: pass 0 reads the SOURCE (log_outer = 0, so in_base = i_first; a one-pass plan has one tile and one column):
  // element `si` of the source column, nothing where si >= n, times zeta^(si mod 3) -- the one extra product, on at
  // most 2n/3 elements of a column.  x is canonical API data (an operand like any unpacked value), zeta's limbs are
  // canonical: the product is in (-p, p/128], normalised (fe29_mul's contract; the header's magnitude paragraph)
  auto load_el = [&](uint32_t j, uint32_t cc) {
    if constexpr (EXT) {
      const uint32_t si = P.is_final ? j : i_first + cc + (j << P.log_inner);
      if (si >= X->n) return Fe29<FP>::zero();
      const Fe29<FP> x = fe29_unpack(fe_load<FP>(xsrc + 2 * (size_t)si));
      const uint32_t r = si % 3;
      if (r == 0) return x;
      return AR::mul(x, fe29_unpack(r == 1 ? X->z1 : X->z2));
    } else if constexpr (DIV) {
      // the plain load times t[i & t_mask]: canonical data, a canonical constant -- EXT's product, on every element
      Fe<FP> t;
      if (Y->t_staged) {
        t = fe_load<FP>(tlds + 2 * (((j & ((1u << Y->t_jbits) - 1)) << P.log_c) + cc));
      } else {
        const uint32_t si = P.is_final ? j : i_first + cc + (j << P.log_inner);
        t = fe_load<FP>(Y->t + 2 * (size_t)(si & Y->t_mask));
#pragma unroll
        for (int d = 0; d < 5; d++) t = fe_dbl(t);
      }
      const Fe29<FP> tv = fe29_unpack(t);
      const Fe29<FP> x = fe29_unpack(fe_load<FP>(src + 2 * (((size_t)j << in_j_shift) + ((size_t)cc << in_c_shift))));
      return AR::mul(x, tv);
    } else {
      return fe29_unpack(fe_load<FP>(src + 2 * (((size_t)j << in_j_shift) + ((size_t)cc << in_c_shift))));
    }
  };
  // one radix-4 group (two fused radix-2 stages s, s + 1) of elements e0..e3 at LDS distance `step`
  auto radix4 = [&](Fe29<FP>& e0, Fe29<FP>& e1, Fe29<FP>& e2, Fe29<FP>& e3, uint32_t s, uint32_t pos) {
    if (s != 0) {                        // s == 0: pos == 0, the twiddles of stage s and of the pair (e0, e2) are 1
      const Fe29<FP> ta = tw_get(pos << (P.log_r - 1 - s));
      e1 = AR::mul(e1, ta);
      e3 = AR::mul(e3, ta);
    }
    const uint32_t tb = pos << (P.log_r - 2 - s);
    const Fe29<FP> a0 = fe29_add(e0, e1), a1 = fe29_sub(e0, e1);
    Fe29<FP> a2 = fe29_add(e2, e3), a3 = fe29_sub(e2, e3);
    if (s != 0) a2 = AR::mul(a2, tw_get(tb));
    // e2 - e3 of two stored values: limbs within +-2^29.  (s == 0 is the stage fused with the tile load: it runs before
    // the block's first barrier, when the LDS copy of the twiddles is still being written -- its one twiddle, the
    // fourth root of unity, comes from the table itself)
    a3 = AR::mul(a3, tw_get(tb + (R >> 2), s == 0));
    e0 = fe29_norm(fe29_add(a0, a2));
    e1 = fe29_norm(fe29_add(a1, a3));
    e2 = fe29_norm(fe29_sub(a0, a2));
    e3 = fe29_norm(fe29_sub(a1, a3));
  };

  // Round 3 (late): the FIRST stage works on the elements as they arrive from HBM and the LAST one hands its results to
  // the exit code in registers -- two of a 1024-row tile's six LDS round trips and two of its six barriers are gone.
  // The thread that owns rows t, t + R/4, t + R/2, t + 3R/4 of the tile (its bit-reversed positions are the four
  // neighbours 4 brev(t) + 0..3) loads them -- consecutive threads still read consecutive addresses, as before.
  // Tiles of fewer than 8 rows (transforms of 2 or 4 elements) keep the plain sequence: load, stages, write back.
  const bool fused = P.log_r >= 3;
  uint32_t s = 0;
  if (fused) {
    if (P.log_r & 1) {
      const uint32_t lq = P.log_r - 1;                   // pairs (t, t + R/2): one radix-2 stage, twiddle 1
      for (uint32_t w = tid; w < (RC >> 1); w += nthr) {
        const uint32_t cc = P.is_final ? w >> lq : w & (C - 1), t = P.is_final ? w & ((1u << lq) - 1) : w >> P.log_c;
        const Fe29<FP> x = load_el(t, cc), y = load_el(t + (R >> 1), cc);
        const uint32_t i0 = (h2_bitrev(t, lq) << (P.log_c + 1)) + cc;
        lds_put(i0, fe29_norm(fe29_add(x, y)));
        lds_put(i0 + C, fe29_norm(fe29_sub(x, y)));
      }
      s = 1;
    } else {
      const uint32_t lq = P.log_r - 2;
      for (uint32_t w = tid; w < (RC >> 2); w += nthr) {
        const uint32_t cc = P.is_final ? w >> lq : w & (C - 1), t = P.is_final ? w & ((1u << lq) - 1) : w >> P.log_c;
        // LDS neighbours q = 0..3 of 4 brev(t) hold rows t + brev2(q) R/4
        Fe29<FP> e0 = load_el(t, cc), e1 = load_el(t + (R >> 1), cc), e2 = load_el(t + (R >> 2), cc),
                 e3 = load_el(t + 3 * (R >> 2), cc);
        radix4(e0, e1, e2, e3, 0, 0);
        const uint32_t i0 = (h2_bitrev(t, lq) << (P.log_c + 2)) + cc;
        lds_put(i0, e0);
        lds_put(i0 + C, e1);
        lds_put(i0 + 2 * C, e2);
        lds_put(i0 + 3 * C, e3);
      }
      s = 2;
    }
    __syncthreads();
  } else {
    // load the tile, bit-reversing j on the way in
    for (uint32_t e = tid; e < RC; e += nthr) {
      const uint32_t j = P.is_final ? e & (R - 1) : e >> P.log_c, cc = P.is_final ? e >> P.log_r : e & (C - 1);
      lds_put((h2_bitrev(j, P.log_r) << P.log_c) + cc, load_el(j, cc));
    }
    __syncthreads();
    if (P.log_r & 1) {
      for (uint32_t w = tid; w < (RC >> 1); w += nthr) {
        const uint32_t cc = w & (C - 1), b = w >> P.log_c;
        const uint32_t i0 = (b << (P.log_c + 1)) + cc, i1 = i0 + C;
        const Fe29<FP> x = lds_get(i0), y = lds_get(i1);
        lds_put(i0, fe29_norm(fe29_add(x, y)));
        lds_put(i1, fe29_norm(fe29_sub(x, y)));
      }
      __syncthreads();
      s = 1;
    }
  }
  const uint32_t s_end = fused ? P.log_r - 2 : P.log_r;
  for (; s < s_end; s += 2) {
    const uint32_t h = 1u << s;
    for (uint32_t w = tid; w < (RC >> 2); w += nthr) {
      const uint32_t cc = w & (C - 1), b = w >> P.log_c;
      const uint32_t pos = b & (h - 1), grp = b >> s;
      const uint32_t i0 = (((grp << (s + 2)) + pos) << P.log_c) + cc;
      const uint32_t step = h << P.log_c;
      Fe29<FP> e0 = lds_get(i0), e1 = lds_get(i0 + step), e2 = lds_get(i0 + 2 * step), e3 = lds_get(i0 + 3 * step);
      radix4(e0, e1, e2, e3, s, pos);
      lds_put(i0, e0);
      lds_put(i0 + step, e1);
      lds_put(i0 + 2 * step, e2);
      lds_put(i0 + 3 * step, e3);
    }
    __syncthreads();
  }
  if (fused) {
    // the last double stage (s = log r - 2: one group, pos = the row): rows pos + q R/4 leave from registers
    const uint32_t step = (R >> 2) << P.log_c;
    for (uint32_t w = tid; w < (RC >> 2); w += nthr) {
      const uint32_t cc = w & (C - 1), pos = w >> P.log_c;
      const uint32_t i0 = (pos << P.log_c) + cc;
      Fe29<FP> e0 = lds_get(i0), e1 = lds_get(i0 + step), e2 = lds_get(i0 + 2 * step), e3 = lds_get(i0 + 3 * step);
      radix4(e0, e1, e2, e3, P.log_r - 2, pos);
      emit(pos, cc, e0);
      emit(pos + (R >> 2), cc, e1);
      emit(pos + 2 * (R >> 2), cc, e2);
      emit(pos + 3 * (R >> 2), cc, e3);
    }
  } else {
    for (uint32_t e = tid; e < RC; e += nthr) emit(e >> P.log_c, e & (C - 1), lds_get(e));
  }
}

template <class FP>
__global__ void __launch_bounds__(1024)
ntt29_pass_kernel(const U128* __restrict__ in, U128* __restrict__ out, const U128* __restrict__ tw,
                  const uint32_t* __restrict__ radix, const int32_t* __restrict__ canon, NttPass P,
                  size_t col_stride /* elements */, Fe<FP> scale29) {
  ntt29_pass_body<FP, false>(in, out, tw, radix, canon, P, col_stride, scale29, nullptr);
}
// pass 0 of an extending transform: `in` is the source (X.src_stride, X.n), `out` has columns of col_stride = 2^P.log_n
template <class FP>
__global__ void __launch_bounds__(1024)
ntt29_extend_pass_kernel(const U128* __restrict__ in, U128* __restrict__ out, const U128* __restrict__ tw,
                         const uint32_t* __restrict__ radix, const int32_t* __restrict__ canon, NttPass P,
                         size_t col_stride /* elements */, NttExtend<FP> X) {
  ntt29_pass_body<FP, true>(in, out, tw, radix, canon, P, col_stride, Fe<FP>::zero(), &X);
}
// extended_to_coeff: DIV = pass 0 multiplies by the t table on the way in, SHR = the final pass keeps Y.out_len outputs
// per column, times zeta^-j (and the scale), in columns Y.out_stride apart.  Both in a one-pass plan
template <class FP, bool DIV, bool SHR>
__global__ void __launch_bounds__(1024)
ntt29_coeff_pass_kernel(const U128* __restrict__ in, U128* __restrict__ out, const U128* __restrict__ tw,
                        const uint32_t* __restrict__ radix, const int32_t* __restrict__ canon, NttPass P,
                        size_t col_stride /* elements */, NttCoeff<FP> Y) {
  ntt29_pass_body<FP, false, DIV, SHR>(in, out, tw, radix, canon, P, col_stride, Fe<FP>::zero(), nullptr, &Y);
}

// ---- host side ------------------------------------------------------------------------------------------------------
inline size_t ntt29_lds_bytes(const NttPass& P) {
  const size_t rc = (size_t)1 << (P.log_r + P.log_c), r = (size_t)1 << P.log_r;
  size_t b = rc * 32 + ((rc * 4 + 15) & ~(size_t)15) + (P.tw_global ? 0 : (r / 2) * 36 + 16);
  return b < 64 ? 64 : b;
}
// a tile that leaves room for a second block on the CU only without its radix twiddles reads them from global memory
// (the 18 KB table of a 1024-row pass stays in the vector L1 / L2)
inline bool ntt29_tw_global(const NttPass& P) {
  static const int tune = tune_int("H2_TUNE_NTT_TWG", -1);     // tuning builds only (h2_tune.hpp)
  if (tune >= 0) return tune != 0;
  const size_t rc = (size_t)1 << (P.log_r + P.log_c), r = (size_t)1 << P.log_r;
  const size_t with = rc * 36 + (r / 2) * 36, without = rc * 36;
  return with > 80 * 1024 && without <= 80 * 1024;
}
// a scaled transform whose constant rides in the inter-pass twiddles (two passes): the table must have been built
// with that constant (ntt29_build_tables(..., scale))
inline bool ntt29_scale_in_table(uint32_t log_n) { return ntt_make_plan(log_n).npass == 2; }

// The dividing pass 0's view of the t table (P = pass 0 with tw_global set; t_mask = period - 1): which row bits reach
// the index's bits below the period, whether the block's C << jbits entries are staged in LDS, where, and the dynamic
// LDS the launch asks for.  Element i = i_first + cc + (j << log_inner) (a one-pass plan: log_inner = log_c = 0).
inline size_t ntt29_div_geometry(const NttPass& P, uint32_t t_mask, uint32_t* jbits, uint32_t* staged, uint32_t* lds_off) {
  uint32_t log_period = 0;
  while ((1u << log_period) <= t_mask && log_period < 31) log_period++;          // period = 2^log_period
  *jbits = log_period > P.log_inner ? std::min(log_period - P.log_inner, P.log_r) : 0;
  const size_t entries = (size_t)1 << (P.log_c + *jbits);
  *staged = entries <= NTT_DIV_LDS_MAX ? 1u : 0u;
  const size_t base = (ntt29_lds_bytes(P) + 15) & ~(size_t)15;
  *lds_off = (uint32_t)(base / 16);
  return *staged ? base + entries * 32 : base;
}
// Every global and LDS index that DIV and SHR add to the plain pass, against its buffer, from the call's shape alone
// (the plain pass's own indices are below 2^log_n in columns 2^log_n apart, as ever).  Null when all is in bounds, else
// what is not.  The caller's buffers: t of t_period elements (has_t), out of (m - 1) * out_stride + out_len.
inline const char* ntt29_coeff_check(uint32_t log_n, size_t out_len, size_t out_stride, bool has_t, size_t t_period, size_t m) {
  if (log_n > 30) return "log_n > 30";
  const size_t n = (size_t)1 << log_n;
  if (m == 0 || m > 65535) return "grid.y = column: 1 <= m <= 65535";
  // SHR stores out[c * out_stride + oi] for oi < out_len only (oi < n is a 32-bit value): the last element written is
  // (m - 1) * out_stride + out_len - 1, and columns do not run into each other
  if (out_len == 0 || out_len > n) return "out_len outside [1, 2^log_n]";
  if (out_stride < out_len) return "out_stride < out_len";
  if (out_stride > ((size_t)1 << 40)) return "out_stride > 2^40";
  if (has_t) {
    // DIV reads t[i & (t_period - 1)]: inside the table for a power of two
    if (t_period == 0 || (t_period & (t_period - 1)) || t_period > n) return "t_period not a power of two in [1, 2^log_n]";
    NttPass P = ntt_make_plan(log_n).pass[0];
    P.tw_global = ntt29_tw_global(P) ? 1u : 0u;
    uint32_t jbits, staged, off;
    const size_t lds = ntt29_div_geometry(P, (uint32_t)(t_period - 1), &jbits, &staged, &off);
    // the staged table: entry ((j & (2^jbits - 1)) << log_c) + cc < C << jbits, 32 bytes each from 16 * off
    if (jbits > P.log_r) return "t_jbits > log_r";
    if (staged && (size_t)16 * off + (((size_t)32 << P.log_c) << jbits) > lds) return "staged t entries beyond the LDS asked for";
    if (lds > 160 * 1024) return "LDS > 160 KB";
  }
  return nullptr;
}

// The passes of one transform of m columns: `in` -> (scratch ->) `out`, columns of n elements in scratch and out.
// ext = null: the plain transform, in's columns are n apart too (ntt29_launch passes in = out).  ext: pass 0 is the
// extending kernel and reads ext->n elements per column, ext->src_stride apart; the later passes are the plain ones.
// co: extended_to_coeff (ntt29_coeff_launch, which has checked the geometry): pass 0 divides when co->t is set, the final
// pass shrinks into out's columns of co->out_stride; a pass that does neither is the plain kernel.
template <class FP>
inline hipError_t ntt29_launch_passes(const U128* in, U128* out, U128* scratch, const void* tables, uint32_t log_n, size_t m,
                                      hipStream_t stream, const Fe<FP>* scale, const NttExtend<FP>* ext,
                                      const NttCoeff<FP>* co = nullptr) {
  NttPlan pl = ntt_make_plan(log_n);
  const NttTables tb = ntt29_tables(log_n);
  const U128* tw = (const U128*)tables;
  const int32_t* canon = (const int32_t*)((const char*)tables + tb.off_canon);
  Fe<FP> sc = scale ? *scale : Fe<FP>::zero();
  for (int d = 0; d < 5; d++) sc = fe_dbl(sc);          // x 2^256 -> x 2^261: the scale as a working-form constant
  const bool in_table = scale && ntt29_scale_in_table(log_n);
  const size_t n = (size_t)1 << log_n;
  for (int p = 0; p < pl.npass; p++) {
    const U128* src;
    U128* dst;
    if (pl.npass == 1) { src = in; dst = out; }
    else if (p == 0) { src = in; dst = scratch; }
    else if (p == pl.npass - 1) { src = scratch; dst = out; }
    else { src = scratch; dst = scratch; }
    dim3 grid(pl.tiles[p], (unsigned)m);
    NttPass P = pl.pass[p];
    P.has_scale = (scale && P.is_final && !in_table) ? 1u : 0u;
    P.tw_global = ntt29_tw_global(P) ? 1u : 0u;
    const uint32_t* radix = (const uint32_t*)((const char*)tables + tb.off_radix[p]);
    static const size_t lds_pad = (size_t)tune_int("H2_TUNE_NTT_LDS_PAD", 0);      // tuning builds: fewer blocks per CU
    const size_t lds = std::min<size_t>(ntt29_lds_bytes(P) + lds_pad, 160 * 1024);
    const bool div = co && co->t && p == 0, shr = co && P.is_final;
    if (div || shr) {
      NttCoeff<FP> Y = *co;
      size_t lds_y = lds;
      if (div) lds_y = ntt29_div_geometry(P, Y.t_mask, &Y.t_jbits, &Y.t_staged, &Y.t_lds_off);
      const dim3 block(pl.threads[p]);
      if (div && shr)
        hipLaunchKernelGGL((ntt29_coeff_pass_kernel<FP, true, true>), grid, block, lds_y, stream, src, dst, tw, radix, canon, P, n, Y);
      else if (div)
        hipLaunchKernelGGL((ntt29_coeff_pass_kernel<FP, true, false>), grid, block, lds_y, stream, src, dst, tw, radix, canon, P, n, Y);
      else
        hipLaunchKernelGGL((ntt29_coeff_pass_kernel<FP, false, true>), grid, block, lds_y, stream, src, dst, tw, radix, canon, P, n, Y);
    } else if (ext && p == 0)
      hipLaunchKernelGGL(ntt29_extend_pass_kernel<FP>, grid, dim3(pl.threads[p]), lds, stream, src, dst, tw, radix, canon, P, n,
                         *ext);
    else
      hipLaunchKernelGGL(ntt29_pass_kernel<FP>, grid, dim3(pl.threads[p]), lds, stream, src, dst, tw, radix, canon, P, n, sc);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}
// Enqueue the transform of m columns (column stride = n elements) on `stream`; data in place, scratch m*n elements
// when the plan has more than one pass; `tables` from ntt29_build_tables; scale (optional) in the API's Montgomery
// form -- with ntt29_scale_in_table(log_n) the tables must carry it.
template <class FP>
inline hipError_t ntt29_launch(U128* data, U128* scratch, const void* tables, uint32_t log_n, size_t m,
                               hipStream_t stream, const Fe<FP>* scale = nullptr) {
  if (log_n == 0 || m == 0) return hipSuccess;
  return ntt29_launch_passes<FP>(data, data, scratch, tables, log_n, m, stream, scale, nullptr);
}
// EvaluationDomain::coeff_to_extended: m source columns of 2^log_src coefficients, src_stride elements apart ->
// out[c][i] = sum_j src[c][j] zeta^j w^(ij) over 2^log_n >= 2^log_src points (zeta^3 = 1, API Montgomery form; tables
// of (w, log_n), unscaled).  Out of place: src is only read; scratch m * 2^log_n elements when the plan has more
// than one pass.  No padded column exists anywhere: pass 0 does not load what would be its zeros.  log_n >= 1.
template <class FP>
inline hipError_t ntt29_extend_launch(const U128* src, size_t src_stride, uint32_t log_src, const Fe<FP>& zeta, U128* out,
                                      U128* scratch, const void* tables, uint32_t log_n, size_t m, hipStream_t stream) {
  if (m == 0) return hipSuccess;
  if (log_n == 0 || log_src > log_n) return hipErrorInvalidValue;
  NttExtend<FP> X;
  X.src_stride = src_stride;
  X.n = 1u << log_src;
  X.z1 = zeta;
  X.z2 = fe_mul(zeta, zeta);
  for (int d = 0; d < 5; d++) {                         // x 2^256 -> x 2^261
    X.z1 = fe_dbl(X.z1);
    X.z2 = fe_dbl(X.z2);
  }
  return ntt29_launch_passes<FP>(src, out, scratch, tables, log_n, m, stream, nullptr, &X);
}
// EvaluationDomain::extended_to_coeff (after divide_by_vanishing_poly when t is given): m columns of 2^log_n values,
// 2^log_n apart, read only ->
//   out[c][j] = zi[j mod 3] * scale * sum_i src[c][i] * t[i mod t_period] * w^(ij)   for j < out_len, zi = {1, zeta_inv, zeta_inv^2}
// in columns out_stride apart; nothing is written at or beyond out_len.  t: t_period canonical elements in the API form,
// or null (no factor).  Tables of (w, log_n), built with `scale` when ntt29_scale_in_table(log_n); scratch m * 2^log_n
// elements when the plan has more than one pass.  log_n = 0 needs no tables.  Every index is checked before the first
// launch (ntt29_coeff_check): hipErrorInvalidValue and nothing enqueued when one is out of bounds.
template <class FP>
inline hipError_t ntt29_coeff_launch(const U128* src, const U128* t, size_t t_period, const Fe<FP>& scale, const Fe<FP>& zeta_inv,
                                     U128* out, size_t out_len, size_t out_stride, U128* scratch, const void* tables,
                                     uint32_t log_n, size_t m, hipStream_t stream) {
  if (m == 0 || out_len == 0) return hipSuccess;
  if (ntt29_coeff_check(log_n, out_len, out_stride, t != nullptr, t_period, m)) return hipErrorInvalidValue;
  NttCoeff<FP> Y{};
  Y.t = t;
  Y.t_mask = t ? (uint32_t)(t_period - 1) : 0;
  Y.out_len = (uint32_t)out_len;
  Y.out_stride = out_stride;
  const Fe<FP> z2 = fe_mul(zeta_inv, zeta_inv);
  if (ntt29_scale_in_table(log_n)) {                    // the final pass has no scale product: 1 (no product), zeta^-1, zeta^-2
    Y.c0 = Fe<FP>::zero();
    Y.c1 = zeta_inv;
    Y.c2 = z2;
  } else {
    Y.c0 = scale;
    Y.c1 = fe_mul(scale, zeta_inv);
    Y.c2 = fe_mul(scale, z2);
  }
  for (int d = 0; d < 5; d++) {                         // x 2^256 -> x 2^261
    Y.c0 = fe_dbl(Y.c0);
    Y.c1 = fe_dbl(Y.c1);
    Y.c2 = fe_dbl(Y.c2);
  }
  return ntt29_launch_passes<FP>(src, out, scratch, tables, log_n, m, stream, &scale, nullptr, &Y);
}
template <class FP>
inline hipError_t ntt29_kernel_setup() {
  const void* kernels[] = {(const void*)ntt29_pass_kernel<FP>, (const void*)ntt29_extend_pass_kernel<FP>,
                           (const void*)ntt29_coeff_pass_kernel<FP, true, false>, (const void*)ntt29_coeff_pass_kernel<FP, false, true>,
                           (const void*)ntt29_coeff_pass_kernel<FP, true, true>};
  for (const void* k : kernels) {
    const hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}
// `tables`: ntt29_tables(log_n).total bytes.  scale (API Montgomery form) or null.
template <class FP>
inline hipError_t ntt29_build_tables(void* tables, const Fe<FP>& omega, uint32_t log_n, hipStream_t stream,
                                     const Fe<FP>* scale = nullptr) {
  if (log_n == 0) return hipSuccess;
  const NttPlan pl = ntt_make_plan(log_n);
  const NttTables tb = ntt29_tables(log_n);
  const uint32_t half_n = 1u << (log_n - 1);
  const uint32_t threads = (half_n + TW_RUN - 1) / TW_RUN;
  const Fe<FP> first = (scale && ntt29_scale_in_table(log_n)) ? *scale : Fe<FP>::one();
  hipLaunchKernelGGL(ntt_twiddle29_kernel<FP>, dim3((threads + 255) / 256), dim3(256), 0, stream, (U128*)tables, omega, first, half_n);
  for (int p = 0; p < pl.npass; p++) {
    const uint32_t half_r = (1u << pl.pass[p].log_r) / 2;
    if (half_r == 0) continue;
    hipLaunchKernelGGL(ntt_radix29_kernel<FP>, dim3((half_r + 255) / 256), dim3(256), 0, stream,
                       (uint32_t*)((char*)tables + tb.off_radix[p]), omega, half_r, log_n - pl.pass[p].log_r);
  }
  hipLaunchKernelGGL(ntt_canon29_kernel<FP>, dim3((NTT_CANON_N + 63) / 64), dim3(64), 0, stream,
                     (int32_t*)((char*)tables + tb.off_canon));
  return hipGetLastError();
}

}  // namespace h2
