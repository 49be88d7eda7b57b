// h2_ipa.hpp -- the inner product argument's rounds on the REGISTERED generators (halo2_proofs @6b43b6b
// src/poly/ipa/commitment/prover.rs `create_proof`, un-vendored; the algorithm is restated in DESIGN.md section 7.13).
//
// Upstream folds three vectors per round: a, b and the generators G' (G'[i] += [u_j] G'[i + half]), and takes L_j, R_j as
// MSMs over the folded G'.  The folded generators are fixed combinations of the original ones,
//     G^(j)[i] = sum_{h < 2^j} s^(j)[h] G[h 2^(k-j) + i],   s^(0) = [1], s^(j+1)[2h] = s^(j)[h], s^(j+1)[2h+1] = s^(j)[h] u_j
// so <a[half..], G^(j)[..half]> is an MSM over the ORIGINAL G with the scalar a[half + i] s^(j)[h] at index
// t = h 2 half + i (and zero at t + half); R_j likewise with a[i] s^(j)[h] at t + half.  No generator is ever folded: a
// round is one two-column MSM of n + 2 terms on the table registered once as G || U || W (slot n: z <a, b>, slot n + 1: the
// blind) plus the kernels below, O(n) field products.
//
// State (caller-owned, IpaBatchLayout; a single opening is a batch of one).  Per opening: a and b in two generations each
// (generation g = a after g folds, 2^(k-g) elements: even generations in a buffer of n, odd ones in a buffer of n / 2 -- the
// round kernel reads one and writes the other, so its threads never race), the table s, one partial pair per workgroup of
// the inner products; behind the openings the two columns of n + 2 of each.
// s is kept in the APPEND-ONLY order S[rev_j(h)] = s^(j)[h] (rev_j: the low j bits reversed): doubling the table is
// S[2^j + g] = S[g] u_j, which reads [0, 2^j) and writes [2^j, 2^(j+1)) -- no race, nothing moves.
//
// Arithmetic: products on the 9 x 29-bit lazy form with the data never converted, as poly_lincomb_kernel (h2_poly.hpp): an
// element in HBM is the integer d = x 2^256 mod p, plain-unpacked; the other factor goes through expr_column_operand,
// c' = c 2^261 + j p in (-16 p, 16 p); fe29_mul(d, c') is x c 2^256 mod p -- the API form of the product -- in (-9p/8, p/8]
// with normalised limbs.  Magnitudes, in units of p (R' = 2^261 > 128 p):
//   * a fold  lo + hi u  is a canonical value plus one product: in (-9p/8, 9p/8), inside w_canonical_pack's (-2p, 2p), so
//     everything stored in a and b is canonical;
//   * a column entry is ONE product, in (-9p/8, p/8]: inside fe29_canonical_pack's (-2p, p);
//   * an inner product: each thread holds one product per sum; 64 lanes add up pairwise (a carry pass per level) to
//     |v| < 72 p, the top limb below 72 * 2^23 < 2^30 and the others normalised: a valid first operand.  One product with
//     the working form of one brings it to (-72p/128 - p, 72p/128]; the four waves' values add up in LDS to (-6.3p, 2.3p)
//     and a second product with one lands in (-1.05p, 0.02p]: canonical_pack.  No atomics; the partials are canonical, so
//     the finishing kernel adds them with the canonical fe_add in a fixed order and the bits do not depend on the grid.
#pragma once
#include "h2_curve_ops.hpp"
#include "h2_field.hpp"
#include "h2_field29.hpp"

#include <cstring>
#include <type_traits>

namespace h2 {

constexpr uint32_t IPA_MAX_K = 20;          // H2_IPA_MAX_K of the C ABI
constexpr int IPA_THREADS = 256;
constexpr uint32_t IPA_H_PER = 2;           // copies (values of h) one thread of the round kernel writes

// The caller's state buffer: m openings of one k in lockstep, in 32-byte elements; a single opening is m = 1.  Opening i
// owns the `per` elements from i * per: a and b in two generations each, S, its partial pairs (a, b, s, partial are offsets
// INSIDE an opening).  Behind the m openings ONE block of 2 m columns at the uniform stride n + 2, ordered L_0, R_0, L_1,
// R_1, ...: one MSM of 2 m columns writes m x (L_i || R_i).  Last the table of per-opening scalars, IPA_BATCH_SCALARS rows of
// m elements, which every call of m >= 2 fills from the host before its kernels (begin: x3, then the m pointers d_p in row 1;
// round: u, 1/u, z, l_blind, r_blind; final: u, 1/u).  At m = 1 the table is there and nothing touches it (IpaOne).
constexpr size_t IPA_MAX_BATCH = 64;        // H2_IPA_MAX_BATCH of the C ABI
constexpr size_t IPA_BATCH_SCALARS = 5;
struct IpaBatchLayout {
  size_t n, hn, m, a[2], b[2], s, partial, partials, per, col, col_stride, scal, total;
  IpaBatchLayout(uint32_t k, size_t m_) {
    n = (size_t)1 << k;
    hn = n / 2;                              // >= 1
    m = m_;
    a[0] = 0;
    a[1] = n;
    b[0] = n + hn;
    b[1] = 2 * n + hn;
    s = 2 * n + 2 * hn;
    partial = 3 * n + 2 * hn;
    partials = (hn + IPA_THREADS - 1) / IPA_THREADS;     // workgroups of the first round that hold an inner product
    per = partial + 2 * partials;
    col = m * per;
    col_stride = n + 2;
    scal = col + 2 * m * col_stride;
    total = scal + IPA_BATCH_SCALARS * m;
  }
};

// The table's rows for a batch of ONE, by value in every kernel's arguments: the call's scalars (Montgomery limbs) and d_p.
// The host fills it instead of the table and enqueues no copy; the kernels take the argument when L.m == 1 (ipa_scalar) --
// unless `table` is set: the route whose scalars are made on the device (h2_ipa_prove.hpp) reads the table at m = 1 too.
struct IpaOne {
  uint32_t v[IPA_BATCH_SCALARS][8];
  const void* p;
  uint32_t table;          // 1: the scalars and d_p come from the state's table whatever m is
  H2_HD bool by_value(size_t m) const { return m == 1 && !table; }
};

// h2_ipa_begin_device: a = p, b[i] = x3^i (each thread POLY_RUN-style runs of 8 from x3^first), S[0] = 1
template <class FP>
__device__ __forceinline__ void ipa_begin_body(const U128* __restrict__ p, U128* __restrict__ a, U128* __restrict__ b,
                                               U128* __restrict__ s, size_t n, const Fe<FP>& x3) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t first = t * 8;
  if (t == 0) fe_store<FP>(s, Fe<FP>::one());
  if (first >= n) return;
  Fe<FP> cur = fe_pow_u64(x3, (uint64_t)first);
  for (int q = 0; q < 8 && first + q < n; q++) {
    fe_store<FP>(a + 2 * (first + q), fe_load<FP>(p + 2 * (first + q)));
    fe_store<FP>(b + 2 * (first + q), cur);
    cur = fe_mul(cur, x3);
  }
}

// the table of challenge products doubles: S[count + g] = S[g] u for g < count.  With set_init (count = 1) S[0] = init
// first: h2_ipa_challenge_products_device runs it k times with u_(k-1), ..., u_0 and gets compute_s in natural order
template <class FP>
__global__ void __launch_bounds__(IPA_THREADS)
ipa_s_kernel(U128* __restrict__ S, uint32_t count, Fe<FP> u, Fe<FP> init, int set_init) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= count) return;
  Fe<FP> x;
  if (set_init) {                      // count == 1
    x = init;
    fe_store<FP>(S, x);
  } else {
    x = fe_load<FP>(S + 2 * (size_t)g);
  }
  fe_store<FP>(S + 2 * ((size_t)count + g), fe_mul(x, u));
}

template <class FP>
struct IpaRound {
  const U128* a_old;       // generation j - 1 (j > 0) or generation 0 (j = 0)
  const U128* b_old;
  U128* a_new;             // generation j (j > 0)
  U128* b_new;
  const U128* S;           // 2^j challenge products, append-only order
  U128* colL;
  U128* colR;
  U128* partial;           // pairs (L, R), one per workgroup that holds an inner product
  Fe<FP> u, uinv;          // u_(j-1) and its inverse (j > 0)
  uint32_t k, j;
};

// Thread T: i = T mod half, hy = T / half.  It forms a'[i], a'[i + half] (from four loads when j > 0), writes the copies
// h in [hy IPA_H_PER, (hy + 1) IPA_H_PER) of its two products into both columns, zeros included, and -- hy = 0 only --
// stores a', b' and adds its two terms to the inner products.
template <class FP>
__device__ __forceinline__ void ipa_round_body(const IpaRound<FP>& A) {
  using F = Fe<FP>;
  using W = Fe29<FP>;
  __shared__ int32_t lds[2][IPA_THREADS / 64][9];
  const uint32_t lh = A.k - A.j - 1;                       // log2(half)
  const size_t half = (size_t)1 << lh;
  const size_t nh = (size_t)1 << A.j;                      // entries of s
  const size_t hy_count = (nh + IPA_H_PER - 1) / IPA_H_PER;
  const size_t T = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t i = T & (half - 1), hy = T >> lh;
  const bool active = hy < hy_count;
  const bool owner = active && hy == 0;                    // T < half
  W ipL = W::zero(), ipR = W::zero();
  if (active) {
    F lo, hi;                                              // a'[i], a'[i + half]
    if (A.j > 0) {
      const W ui = expr_column_operand(A.uinv);
      const F a0 = fe_load<FP>(A.a_old + 2 * i), a1 = fe_load<FP>(A.a_old + 2 * (i + half));
      const F a2 = fe_load<FP>(A.a_old + 2 * (i + 2 * half)), a3 = fe_load<FP>(A.a_old + 2 * (i + 3 * half));
      lo = w_canonical_pack(fe29_add(fe29_unpack(a0), fe29_mul(fe29_unpack(a2), ui)));
      hi = w_canonical_pack(fe29_add(fe29_unpack(a1), fe29_mul(fe29_unpack(a3), ui)));
    } else {
      lo = fe_load<FP>(A.a_old + 2 * i);
      hi = fe_load<FP>(A.a_old + 2 * (i + half));
    }
    if (owner) {
      F blo, bhi;
      if (A.j > 0) {
        const W uu = expr_column_operand(A.u);
        const F b0 = fe_load<FP>(A.b_old + 2 * i), b1 = fe_load<FP>(A.b_old + 2 * (i + half));
        const F b2 = fe_load<FP>(A.b_old + 2 * (i + 2 * half)), b3 = fe_load<FP>(A.b_old + 2 * (i + 3 * half));
        blo = w_canonical_pack(fe29_add(fe29_unpack(b0), fe29_mul(fe29_unpack(b2), uu)));
        bhi = w_canonical_pack(fe29_add(fe29_unpack(b1), fe29_mul(fe29_unpack(b3), uu)));
        fe_store<FP>(A.a_new + 2 * i, lo);
        fe_store<FP>(A.a_new + 2 * (i + half), hi);
        fe_store<FP>(A.b_new + 2 * i, blo);
        fe_store<FP>(A.b_new + 2 * (i + half), bhi);
      } else {
        blo = fe_load<FP>(A.b_old + 2 * i);
        bhi = fe_load<FP>(A.b_old + 2 * (i + half));
      }
      ipL = fe29_mul(fe29_unpack(hi), expr_column_operand(blo));     // <a[half..], b[..half]>
      ipR = fe29_mul(fe29_unpack(lo), expr_column_operand(bhi));     // <a[..half], b[half..]>
    }
    const W wlo = fe29_unpack(lo), whi = fe29_unpack(hi);
    const F zero = F::zero();
    for (uint32_t q = 0; q < IPA_H_PER; q++) {
      const size_t h = hy * IPA_H_PER + q;
      if (h >= nh) break;
      const uint32_t idx = A.j ? (__brev((uint32_t)h) >> (32 - A.j)) : 0u;
      const W sh = expr_column_operand(fe_load<FP>(A.S + 2 * (size_t)idx));
      const size_t t = h * 2 * half + i;
      fe_store<FP>(A.colL + 2 * t, fe29_canonical_pack(fe29_mul(whi, sh)));
      fe_store<FP>(A.colL + 2 * (t + half), zero);
      fe_store<FP>(A.colR + 2 * t, zero);
      fe_store<FP>(A.colR + 2 * (t + half), fe29_canonical_pack(fe29_mul(wlo, sh)));
    }
  }
  if ((size_t)blockIdx.x * blockDim.x >= half) return;     // uniform: this workgroup holds no inner product term
  // in the wave (64 lanes): pairwise, a carry pass per level
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    W oL, oR;
#pragma unroll
    for (int l = 0; l < 9; l++) {
      oL.v[l] = __shfl_xor(ipL.v[l], d, 64);
      oR.v[l] = __shfl_xor(ipR.v[l], d, 64);
    }
    ipL = fe29_norm(fe29_add(ipL, oL));
    ipR = fe29_norm(fe29_add(ipR, oR));
  }
  const W one = fe29_from_api(F::one());
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0) {
    const W vL = fe29_mul(ipL, one), vR = fe29_mul(ipR, one);
#pragma unroll
    for (int l = 0; l < 9; l++) {
      lds[0][wave][l] = vL.v[l];
      lds[1][wave][l] = vR.v[l];
    }
  }
  __syncthreads();
  if (threadIdx.x < 2) {                                   // thread 0: L, thread 1: R
    W acc = W::zero();
    for (int w = 0; w < IPA_THREADS / 64; w++) {
#pragma unroll
      for (int l = 0; l < 9; l++) acc.v[l] += lds[threadIdx.x][w][l];
    }
    fe_store<FP>(A.partial + 2 * ((size_t)blockIdx.x * 2 + threadIdx.x), fe29_canonical_pack(fe29_mul(fe29_norm(acc), one)));
  }
}

// one workgroup: the sums of the `count` partial pairs times z into slot n of the columns, the blinds into slot n + 1
template <class FP>
__device__ __forceinline__ void ipa_finish_body(const U128* __restrict__ partial, uint32_t count, const Fe<FP>& z,
                                                const Fe<FP>& l_blind, const Fe<FP>& r_blind, U128* __restrict__ tailL,
                                                U128* __restrict__ tailR) {
  using F = Fe<FP>;
  __shared__ uint32_t lds[2][8][IPA_THREADS];              // [sum][limb][thread]
  const uint32_t t = threadIdx.x;
  F acc[2] = {F::zero(), F::zero()};
  for (uint32_t p = t; p < count; p += IPA_THREADS) {
    acc[0] = fe_add(acc[0], fe_load<FP>(partial + 2 * ((size_t)p * 2)));
    acc[1] = fe_add(acc[1], fe_load<FP>(partial + 2 * ((size_t)p * 2 + 1)));
  }
  for (uint32_t st = IPA_THREADS / 2; st >= 1; st >>= 1) {
#pragma unroll
    for (int c = 0; c < 2; c++)
#pragma unroll
      for (int l = 0; l < 8; l++) lds[c][l][t] = acc[c].v[l];
    __syncthreads();
    if (t < st) {
#pragma unroll
      for (int c = 0; c < 2; c++) {
        F o;
#pragma unroll
        for (int l = 0; l < 8; l++) o.v[l] = lds[c][l][t + st];
        acc[c] = fe_add(acc[c], o);
      }
    }
    __syncthreads();
  }
  if (t == 0) {
    fe_store<FP>(tailL, fe_mul(acc[0], z));
    fe_store<FP>(tailL + 2, l_blind);
    fe_store<FP>(tailR, fe_mul(acc[1], z));
    fe_store<FP>(tailR + 2, r_blind);
  }
}

// h2_ipa_final_device: the last fold, c = a[0] + a[1] / u and b[0] + b[1] u (thread 0), and the finished table in natural
// order, s[i] = S[rev_k(i)], when the caller wants it
template <class FP>
__device__ __forceinline__ void ipa_final_body(const U128* __restrict__ a, const U128* __restrict__ b, const U128* __restrict__ S,
                                               const Fe<FP>& u, const Fe<FP>& uinv, uint32_t k, U128* __restrict__ out,
                                               U128* __restrict__ s_out) {
  const size_t T = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (T == 0) {
    fe_store<FP>(out, fe_add(fe_load<FP>(a), fe_mul(fe_load<FP>(a + 2), uinv)));
    fe_store<FP>(out + 2, fe_add(fe_load<FP>(b), fe_mul(fe_load<FP>(b + 2), u)));
  }
  if (s_out && T < ((size_t)1 << k))
    fe_store<FP>(s_out + 2 * T, fe_load<FP>(S + 2 * (size_t)(__brev((uint32_t)T) >> (32 - k))));
}

// ---- the kernels: blockIdx.y is the opening, blockIdx.x what the bodies above take it for -----------------------------------
// An opening's scalars come from the table at the end of the state (IpaBatchLayout), or at m = 1 from the kernel's
// arguments (IpaOne) unless one.table says otherwise; both are arguments, so the choice is uniform across the launch.  No kernel writes the table and a
// workgroup works on one opening, so the table address is the same in every lane: the loads go through the constant
// address space, which the back end serves with scalar loads (poseidon_const's way), as it does the arguments.
template <class FP>
__device__ __forceinline__ Fe<FP> ipa_scalar(const U128* st, const IpaBatchLayout& L, const IpaOne& one, size_t row,
                                             size_t opening) {
  typedef const __attribute__((address_space(4))) uint32_t* ConstPtr;
  const ConstPtr q = (ConstPtr)(const uint32_t*)(st + 2 * (L.scal + row * L.m + opening));
  Fe<FP> r;
#pragma unroll
  for (int l = 0; l < 8; l++) r.v[l] = one.by_value(L.m) ? one.v[row][l] : q[l];
  return r;
}

template <class FP>
__global__ void __launch_bounds__(IPA_THREADS) ipa_begin_kernel(U128* st, IpaBatchLayout L, IpaOne one) {
  const size_t o = blockIdx.y;
  typedef const __attribute__((address_space(4))) uint64_t* ConstPtr;
  typedef const __attribute__((address_space(1))) U128* GlobalPtr;       // d_p[o] is device memory: global loads, not flat ones
  const uintptr_t p = one.by_value(L.m) ? (uintptr_t)one.p : (uintptr_t)((ConstPtr)(const uint64_t*)(st + 2 * (L.scal + L.m)))[o];
  U128* base = st + 2 * o * L.per;
  ipa_begin_body<FP>((const U128*)(GlobalPtr)p, base + 2 * L.a[0], base + 2 * L.b[0], base + 2 * L.s, L.n,
                     ipa_scalar<FP>(st, L, one, 0, o));
}

// S[count + g] = S[g] u per opening: ipa_s_kernel's doubling without its set_init form
template <class FP>
__global__ void __launch_bounds__(IPA_THREADS) ipa_s_double_kernel(U128* st, IpaBatchLayout L, IpaOne one, uint32_t count) {
  const size_t o = blockIdx.y;
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= count) return;
  U128* S = st + 2 * (o * L.per + L.s);
  fe_store<FP>(S + 2 * ((size_t)count + g), fe_mul(fe_load<FP>(S + 2 * (size_t)g), ipa_scalar<FP>(st, L, one, 0, o)));
}

template <class FP>
__global__ void __launch_bounds__(IPA_THREADS) ipa_round_kernel(U128* st, IpaBatchLayout L, IpaOne one, uint32_t k, uint32_t j) {
  const size_t o = blockIdx.y;
  U128* base = st + 2 * o * L.per;
  IpaRound<FP> A;
  A.k = k;
  A.j = j;
  A.S = base + 2 * L.s;
  A.colL = st + 2 * (L.col + 2 * o * L.col_stride);
  A.colR = A.colL + 2 * L.col_stride;
  A.partial = base + 2 * L.partial;
  if (j > 0) {
    A.u = ipa_scalar<FP>(st, L, one, 0, o);
    A.uinv = ipa_scalar<FP>(st, L, one, 1, o);
    A.a_old = base + 2 * L.a[(j - 1) & 1];
    A.b_old = base + 2 * L.b[(j - 1) & 1];
    A.a_new = base + 2 * L.a[j & 1];
    A.b_new = base + 2 * L.b[j & 1];
  } else {
    A.u = A.uinv = Fe<FP>::zero();
    A.a_old = base + 2 * L.a[0];
    A.b_old = base + 2 * L.b[0];
    A.a_new = nullptr;
    A.b_new = nullptr;
  }
  ipa_round_body<FP>(A);
}

template <class FP>
__global__ void __launch_bounds__(IPA_THREADS) ipa_finish_kernel(U128* st, IpaBatchLayout L, IpaOne one, uint32_t count) {
  const size_t o = blockIdx.y;
  U128* colL = st + 2 * (L.col + 2 * o * L.col_stride);
  ipa_finish_body<FP>(st + 2 * (o * L.per + L.partial), count, ipa_scalar<FP>(st, L, one, 2, o), ipa_scalar<FP>(st, L, one, 3, o),
                      ipa_scalar<FP>(st, L, one, 4, o), colL + 2 * L.n, colL + 2 * (L.col_stride + L.n));
}

// out: m x (c_i || b_i[0]); s_out (or null): m x the finished table of n elements
template <class FP>
__global__ void __launch_bounds__(IPA_THREADS)
ipa_final_kernel(const U128* st, IpaBatchLayout L, IpaOne one, uint32_t k, U128* out, U128* s_out) {
  const size_t o = blockIdx.y;
  const U128* base = st + 2 * o * L.per;
  ipa_final_body<FP>(base + 2 * L.a[(k - 1) & 1], base + 2 * L.b[(k - 1) & 1], base + 2 * L.s, ipa_scalar<FP>(st, L, one, 0, o),
                     ipa_scalar<FP>(st, L, one, 1, o), k, out + 4 * o, s_out ? s_out + 2 * o * L.n : nullptr);
}

// ---- launches (one per curve through CurveOps) ----------------------------------------------------------------------------
template <class FP>
inline Fe<FP> ipa_fe(const uint64_t* limbs) {
  Fe<FP> r;
  memcpy(r.v, limbs, 32);
  return r;
}

// the launches: for m >= 2 the caller has copied the call's scalar table into the state on `s` (IpaBatchLayout), for m = 1 it
// has filled `one`; one launch of each kernel serves the m openings
template <class FP>
hipError_t ipa_begin_batch_launch(uint32_t k, size_t m, const IpaOne& one, void* d_state, hipStream_t s) {
  const IpaBatchLayout L(k, m);
  const size_t threads = (L.n + 7) / 8;
  hipLaunchKernelGGL(ipa_begin_kernel<FP>, dim3((unsigned)((threads + IPA_THREADS - 1) / IPA_THREADS), (unsigned)m), dim3(IPA_THREADS), 0, s,
                     (U128*)d_state, L, one);
  return hipGetLastError();
}

template <class FP>
hipError_t ipa_round_batch_launch(uint32_t k, uint32_t j, size_t m, const IpaOne& one, void* d_state, hipStream_t s) {
  const IpaBatchLayout L(k, m);
  U128* st = (U128*)d_state;
  if (j > 0) {
    const uint32_t count = 1u << (j - 1);
    hipLaunchKernelGGL(ipa_s_double_kernel<FP>, dim3((count + IPA_THREADS - 1) / IPA_THREADS, (unsigned)m), dim3(IPA_THREADS), 0, s, st, L,
                       one, count);
  }
  const size_t half = (size_t)1 << (k - j - 1), nh = (size_t)1 << j;
  const size_t threads = half * ((nh + IPA_H_PER - 1) / IPA_H_PER);
  hipLaunchKernelGGL(ipa_round_kernel<FP>, dim3((unsigned)((threads + IPA_THREADS - 1) / IPA_THREADS), (unsigned)m), dim3(IPA_THREADS), 0,
                     s, st, L, one, k, j);
  const uint32_t parts = (uint32_t)((half + IPA_THREADS - 1) / IPA_THREADS);
  hipLaunchKernelGGL(ipa_finish_kernel<FP>, dim3(1, (unsigned)m), dim3(IPA_THREADS), 0, s, st, L, one, parts);
  return hipGetLastError();
}

// the last doubling of S only when the finished table is asked for: nothing else reads it any more
template <class FP>
hipError_t ipa_final_batch_launch(uint32_t k, size_t m, const IpaOne& one, void* d_state, void* d_out, void* d_s_out, hipStream_t s) {
  const IpaBatchLayout L(k, m);
  U128* st = (U128*)d_state;
  if (d_s_out) {
    const uint32_t count = 1u << (k - 1);
    hipLaunchKernelGGL(ipa_s_double_kernel<FP>, dim3((count + IPA_THREADS - 1) / IPA_THREADS, (unsigned)m), dim3(IPA_THREADS), 0, s, st, L,
                       one, count);
  }
  const size_t threads = d_s_out ? L.n : 1;
  hipLaunchKernelGGL(ipa_final_kernel<FP>, dim3((unsigned)((threads + IPA_THREADS - 1) / IPA_THREADS), (unsigned)m), dim3(IPA_THREADS), 0,
                     s, (const U128*)st, L, one, k, (U128*)d_out, (U128*)d_s_out);
  return hipGetLastError();
}

// compute_s(u, init) into d_out (2^k elements): k doublings, the challenges taken from the last to the first
template <class FP>
hipError_t ipa_s_products_launch(const uint64_t* u, uint32_t k, const uint64_t init[4], void* d_out, hipStream_t s) {
  const Fe<FP> in = ipa_fe<FP>(init);
  for (uint32_t t = 0; t < k; t++) {
    const uint32_t count = 1u << t;
    hipLaunchKernelGGL(ipa_s_kernel<FP>, dim3((count + IPA_THREADS - 1) / IPA_THREADS), dim3(IPA_THREADS), 0, s, (U128*)d_out, count,
                       ipa_fe<FP>(u + 4 * (k - 1 - t)), in, t == 0 ? 1 : 0);
  }
  return hipGetLastError();
}

// ---- the weighted sum of challenge-product vectors (h2_ipa_challenge_products_sum_device) -----------------------------------
// out[i] = sum_p init_p prod_{bit t of i} u_p[k-1-t]: what a batch verifier needs of `count` compute_s vectors -- their sum,
// the N final equations being linear in the same table -- without any of them in memory.
//
// A thread owns the run of 2^4 consecutive indices [16 T, 16 T + 16).  Per proof it forms the product over the HIGH k - 4 bits
// of its run (the proof's table entry is the same for the whole launch: scalar loads; the multiplier is a select between
// u and one, the bits differ inside a wave), expands the run depth-first with 2^4 - 1 products (bit t of the index
// multiplies by u[k-1-t]) and adds the sixteen values into sixteen lazy accumulators: (k - 4 + 15) / 16 < 2 products per
// element and proof for k <= 20.  For k < 4 the levels from k up multiply by one and the indices from 2^k up are not
// stored (r = min(4, k) with the missing levels padded: a launch of one thread, 15 products per proof whatever k).
//
// The table (host-made, ipa_sum_fill, in the scan arena for the length of the call): per proof the canonical init (8
// words) and max(k, 4) multipliers, level t holding u[k-1-t] (one for t >= k) as expr_column_operand makes it, 9 limbs.
//
// Arithmetic as poly_lincomb_kernel's: d (canonical, plain-unpacked: x 2^256 mod p) times c' (the operand form, in
// (-16 p, 16 p)) is d c' / R' - m p, the API form of the product.  With |d| <= B the result lies in (-B / 8 - p, B / 8]
// (R' > 128 p), so a chain of such products that starts from a canonical value stays in (-8p/7, p/7], limbs normalised.
// The accumulators, in units of p:
//   * a term is added limb-wise; after every SECOND proof one carry pass: a normalised sum plus two normalised terms has
//     limbs below 3 * 2^29 < 2^31;
//   * every IPA_SUM_FOLD = 32 proofs the sum is multiplied by the working form of one: unchanged mod p, it falls below
//     |acc| / 128 + p.  Between folds |acc| < 1.4 p + 32 * 8p/7 < 38.2 p (a later group starts from the canonical value
//     already in d_out instead: < p + 36.6 p), the top limb below 39 * 2^23 < 2^29: a valid operand;
//   * the last product with one lands in (-39p/128 - p, 39p/128], inside fe29_canonical_pack's (-2p, p).  The stored limbs
//     are canonical, so the bits do not depend on how the proofs were grouped.  No atomics: an output has one owner.
constexpr uint32_t IPA_SUM_RUN_LOG = 4;
constexpr uint32_t IPA_SUM_FOLD = 32;
constexpr size_t IPA_SUM_GROUP = 65535;                   // proofs per launch
constexpr int IPA_SUM_THREADS = 64;
static_assert(IPA_SUM_FOLD % 2 == 0, "the fold follows a carry pass");

inline uint32_t ipa_sum_levels(uint32_t k) { return k > IPA_SUM_RUN_LOG ? k : IPA_SUM_RUN_LOG; }
inline uint32_t ipa_sum_stride(uint32_t k) { return 8 + 9 * ipa_sum_levels(k); }     // 32-bit words per proof

// the table of `count` proofs at out: u count * k * 4 limbs, init count * 4 limbs, canonical Montgomery
template <class FP>
void ipa_sum_fill(const uint64_t* u, const uint64_t* init, uint32_t k, size_t count, int32_t* out) {
  const uint32_t levels = ipa_sum_levels(k), stride = ipa_sum_stride(k);
  const Fe29<FP> one = expr_column_operand(Fe<FP>::one());
  for (size_t p = 0; p < count; p++) {
    int32_t* row = out + p * stride;
    memcpy(row, init + 4 * p, 32);
    for (uint32_t t = 0; t < levels; t++) {
      const Fe29<FP> m = t < k ? expr_column_operand(ipa_fe<FP>(u + 4 * (p * k + (k - 1 - t)))) : one;
      memcpy(row + 8 + 9 * t, m.v, 36);
    }
  }
}

// fn(integral_constant<int, 0>) ... fn(integral_constant<int, N - 1>): the accumulators are indexed by constants from the
// front end on, so they are registers whatever the unroller decides
template <int N, class Fn>
H2_HD void ipa_static_for(Fn&& fn) {
  if constexpr (N > 0) {
    ipa_static_for<N - 1>(fn);
    fn(std::integral_constant<int, N - 1>{});
  }
}

// the run below `val` (the product over the levels from LEVEL up): level t - 1 multiplies the upper half by op[t - 1]
template <class FP, int LEVEL, int IDX>
__device__ __forceinline__ void ipa_sum_expand(const Fe29<FP>& val, const Fe29<FP>* op, Fe29<FP>* acc) {
  if constexpr (LEVEL == 0) {
    acc[IDX] = fe29_add(acc[IDX], val);
  } else {
    ipa_sum_expand<FP, LEVEL - 1, IDX>(val, op, acc);
    ipa_sum_expand<FP, LEVEL - 1, IDX + (1 << (LEVEL - 1))>(fe29_mul(val, op[LEVEL - 1]), op, acc);
  }
}

template <class FP>
__global__ void __launch_bounds__(IPA_SUM_THREADS)
ipa_s_sum_kernel(const int32_t* __restrict__ table, uint32_t stride, uint32_t count, uint32_t k, U128* out, int accumulate) {
  using F = Fe<FP>;
  using W = Fe29<FP>;
  constexpr int RUN = 1 << IPA_SUM_RUN_LOG;
  const size_t n = (size_t)1 << k;
  const size_t T = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t first = T * RUN;
  if (first >= n) return;
  const W one = fe29_from_api(F::one()), one_op = expr_column_operand(F::one());
  W acc[RUN];
  ipa_static_for<RUN>([&](auto g) {
    acc[g] = accumulate && first + g < n ? fe29_unpack(fe_load<FP>(out + 2 * (first + g))) : W::zero();
  });
  for (uint32_t p = 0; p < count; p++) {
    const int32_t* __restrict__ row = table + (size_t)p * stride;
    F init;
#pragma unroll
    for (int l = 0; l < 8; l++) init.v[l] = (uint32_t)row[l];
    auto level = [&](uint32_t t) {
      W m;
#pragma unroll
      for (int l = 0; l < 9; l++) m.v[l] = row[8 + 9 * t + l];
      return m;
    };
    W val = fe29_unpack(init);
    for (uint32_t t = IPA_SUM_RUN_LOG; t < k; t++) {
      const W m = level(t);
      const bool set = (T >> (t - IPA_SUM_RUN_LOG)) & 1;
      W sel;
#pragma unroll
      for (int l = 0; l < 9; l++) sel.v[l] = set ? m.v[l] : one_op.v[l];
      val = fe29_mul(val, sel);
    }
    W op[IPA_SUM_RUN_LOG];
#pragma unroll
    for (uint32_t t = 0; t < IPA_SUM_RUN_LOG; t++) op[t] = level(t);
    ipa_sum_expand<FP, (int)IPA_SUM_RUN_LOG, 0>(val, op, acc);
    if (p & 1) {
      ipa_static_for<RUN>([&](auto g) { acc[g] = fe29_norm(acc[g]); });
      if ((p + 1) % IPA_SUM_FOLD == 0) ipa_static_for<RUN>([&](auto g) { acc[g] = fe29_mul(acc[g], one); });
    }
  }
  ipa_static_for<RUN>([&](auto g) {
    if (first + g < n) fe_store<FP>(out + 2 * (first + g), fe29_canonical_pack(fe29_mul(fe29_norm(acc[g]), one)));
  });
}

template <class FP>
hipError_t ipa_s_sum_launch(const void* d_table, uint32_t count, uint32_t k, void* d_out, bool accumulate, hipStream_t s) {
  const size_t threads = (((size_t)1 << k) + (1u << IPA_SUM_RUN_LOG) - 1) >> IPA_SUM_RUN_LOG;
  hipLaunchKernelGGL(ipa_s_sum_kernel<FP>, dim3((unsigned)((threads + IPA_SUM_THREADS - 1) / IPA_SUM_THREADS)), dim3(IPA_SUM_THREADS), 0, s,
                     (const int32_t*)d_table, ipa_sum_stride(k), count, k, (U128*)d_out, accumulate ? 1 : 0);
  return hipGetLastError();
}

}  // namespace h2
