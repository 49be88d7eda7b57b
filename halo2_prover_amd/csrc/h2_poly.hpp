// h2_poly.hpp -- pointwise polynomial kernels around the NTT: the device pieces of
// halo2_proofs::poly::EvaluationDomain (halo2_proofs @6b43b6b, src/poly/domain.rs -- un-vendored; behaviour
// restated in SURVEY.md App. A.3; reached from /root/reference/circuits/src/utils.rs:83-91,105-120 through
// create_proof): ifft's n^-1 scaling, distribute_powers_zeta (the coset shift a[i] *= g^i),
// divide_by_vanishing_poly (a[i] *= t[i mod period]) and the pointwise add / sub / mul of evaluate_h.
// All are one read + one write of the column: HBM-bound elementwise kernels (64 B per element), kept on
// device so a column never leaves HBM between its NTTs and its MSM.
#pragma once
#include "h2_curve_ops.hpp"
#include "h2_field.hpp"
#include "h2_field29.hpp"

namespace h2 {

constexpr int POLY_RUN = 8;  // consecutive elements per thread in the powers kernel

// a[i] *= c   (m columns, stride n)
template <class FP>
__global__ void __launch_bounds__(256) poly_scale_kernel(U128* __restrict__ a, size_t total, Fe<FP> c) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    Fe<FP> x = fe_load<FP>(a + 2 * i);
    fe_store<FP>(a + 2 * i, fe_mul(x, c));
  }
}

// a[col][i] *= g^i : each thread owns POLY_RUN consecutive i, starts from g^(first i) by square-and-multiply
template <class FP>
__global__ void __launch_bounds__(256)
poly_powers_kernel(U128* __restrict__ a, size_t n, Fe<FP> g) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t first = t * POLY_RUN;
  if (first >= n) return;
  U128* col = a + 2 * n * blockIdx.y;
  Fe<FP> cur = fe_pow_u64(g, (uint64_t)first);
  for (int k = 0; k < POLY_RUN && first + k < n; k++) {
    Fe<FP> x = fe_load<FP>(col + 2 * (first + k));
    fe_store<FP>(col + 2 * (first + k), fe_mul(x, cur));
    cur = fe_mul(cur, g);
  }
}

// a[col][i] *= t[i mod period]  (period a power of two)
template <class FP>
__global__ void __launch_bounds__(256)
poly_mul_periodic_kernel(U128* __restrict__ a, size_t total, const U128* __restrict__ t, size_t period_mask) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    Fe<FP> x = fe_load<FP>(a + 2 * i);
    Fe<FP> y = fe_load<FP>(t + 2 * (i & period_mask));
    fe_store<FP>(a + 2 * i, fe_mul(x, y));
  }
}

// a[i] = a[i] (op) b[i],  op: 0 add, 1 sub, 2 mul
template <class FP>
__global__ void __launch_bounds__(256)
poly_pointwise_kernel(U128* __restrict__ a, const U128* __restrict__ b, size_t total, int op) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    Fe<FP> x = fe_load<FP>(a + 2 * i), y = fe_load<FP>(b + 2 * i), r;
    if (op == 0) r = fe_add(x, y);
    else if (op == 1) r = fe_sub(x, y);
    else r = fe_mul(x, y);
    fe_store<FP>(a + 2 * i, r);
  }
}

// a[i] = a[i]^-1 (0 stays 0): the denominators of the permutation grand product.  The is_zero test is not what keeps a
// zero: fe_inv(0) = 0^(p-2) is canonical 0 anyway (the chain's first multiplication is by a); it only saves the
// exponentiation and the store
template <class FP>
__global__ void __launch_bounds__(256) poly_inverse_kernel(U128* __restrict__ a, size_t total) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    Fe<FP> x = fe_load<FP>(a + 2 * i);
    if (!x.is_zero()) fe_store<FP>(a + 2 * i, fe_inv(x));
  }
}

// ---- kate_division and the exclusive prefix product, several in ONE launch sequence (grid.y = job) --------------------
// mode 0: q = (a - a(z)) / (X - z), halo2_proofs @6b43b6b src/arithmetic.rs `kate_division` (called by the GWC / SHPLONK
// provers on every opened polynomial): the serial recurrence q[i-1] = a[i] + z q[i] from the top coefficient down,
// q[n-1] = 0.  Written Q_i = sum_{j >= i} a[j] z^(j-i) it is a suffix sum with weights.  out != a.
// mode 1: out[i] = prod_{j < i} a[j], out[0] = 1.  The permutation argument's grand product (halo2_proofs @6b43b6b
// src/plonk/permutation/prover.rs `Argument::commit`: z[0] = last_z, z[i+1] = z[i] * numerator[i] / denominator[i]) is
// this scan of the per-row ratios, times last_z.  May run in place (a thread reads a[i] before it writes out[i]).
// Three launches over C <= SCAN_CHUNKS chunks of L >= 16 elements: each chunk's own value, a scan of the chunk values in
// one block (for the division with multiplier w = z^L), then the recurrence inside every chunk started from the scanned
// value.  Each scan is a latency chain on 16 waves; independent jobs side by side (the opening witnesses of the GWC
// points, the permutation sets' grand products) cost what one costs.  Scratch: SCAN_WS_BYTES per job.
constexpr int SCAN_MAX_JOBS = 8;
constexpr uint32_t SCAN_CHUNKS = 4096;
constexpr size_t SCAN_WS_BYTES = 2 * SCAN_CHUNKS * 32;   // the chunk values H and the scanned values G
template <class FP>
struct ScanBatch {
  const U128* a[SCAN_MAX_JOBS];
  U128* out[SCAN_MAX_JOBS];
  Fe<FP> z[SCAN_MAX_JOBS];   // division only: the point
  Fe<FP> w[SCAN_MAX_JOBS];   // division only: z^L
};
// Both modes on the 29-bit form (a chain of products on one wave: twice as fast there).  Mode 1 works on true values:
// loads through expr_column_operand, one extra product (fe29_to_api) per stored element, off the chain.  Mode 0 is
// LINEAR in the data, so the data stay in the API's form read as the working form of x / 32 (plain unpack, no conversion
// either way): with z in the true working form, acc z / R' + a keeps that scaling, and a result only needs to be made
// canonical to be stored.
constexpr int SCAN_AHEAD = 4;     // elements loaded ahead of the recurrence (the chain itself cannot hide a load)
template <class FP>
__global__ void __launch_bounds__(64)
poly_scan_chunk_kernel(ScanBatch<FP> B, int mode, size_t n, uint32_t L, uint32_t C, U128* __restrict__ H) {
  using F = Fe<FP>;
  using W = Fe29<FP>;
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x, job = blockIdx.y;
  if (c >= C) return;
  const U128* a = B.a[job];
  const size_t lo = (size_t)c * L, hi = min(n, lo + L);
  U128* dst = H + 2 * ((size_t)job * SCAN_CHUNKS + c);
  if (mode == 0) {
    W acc = W::zero();
    const W z = expr_column_operand(B.z[job]);
    for (size_t top = hi; top > lo;) {
      const uint32_t cnt = (uint32_t)min((size_t)SCAN_AHEAD, top - lo);
      F v[SCAN_AHEAD];
#pragma unroll
      for (int k = 0; k < SCAN_AHEAD; k++)
        if ((uint32_t)k < cnt) v[k] = fe_load<FP>(a + 2 * (top - 1 - k));
#pragma unroll
      for (int k = 0; k < SCAN_AHEAD; k++)
        if ((uint32_t)k < cnt) acc = fe29_add(fe29_mul(acc, z), fe29_unpack(v[k]));
      top -= cnt;
    }
    fe_store<FP>(dst, w_canonical_pack(acc));
  } else {
    W acc = fe29_from_api(F::one());
    for (size_t at = lo; at < hi;) {
      const uint32_t cnt = (uint32_t)min((size_t)SCAN_AHEAD, hi - at);
      F v[SCAN_AHEAD];
#pragma unroll
      for (int k = 0; k < SCAN_AHEAD; k++)
        if ((uint32_t)k < cnt) v[k] = fe_load<FP>(a + 2 * (at + k));
#pragma unroll
      for (int k = 0; k < SCAN_AHEAD; k++)
        if ((uint32_t)k < cnt) acc = fe29_mul(acc, expr_column_operand(v[k]));
      at += cnt;
    }
    fe_store<FP>(dst, fe29_to_api(acc));
  }
}
// Scan of the C <= SCAN_CHUNKS chunk values in one block of SCAN_BLOCK_THREADS threads: every thread takes
// SCAN_PER_THREAD consecutive values (a short recurrence in registers), the group totals go through a log-step scan
// in LDS (unpacked, 36 bytes each), and the thread finishes its own values.  The block is a chain of products on ONE
// CU: measured 69 us with 1024 threads x 4 values (16 waves queue for four SIMDs), 74 us with 256 x 16 (long local
// recurrences), 61 us with 512 x 8.  With 4096 chunks of 16 elements the three kernels take 17 + 61 + 28 us for the
// four opening quotients of a proof; with 1024 chunks of 64 they took 58 + 40 + 65.
constexpr int SCAN_BLOCK_THREADS = 512;
constexpr int SCAN_PER_THREAD = SCAN_CHUNKS / SCAN_BLOCK_THREADS;
template <class FP>
__global__ void __launch_bounds__(SCAN_BLOCK_THREADS)
poly_scan_block_kernel(ScanBatch<FP> B, int mode, uint32_t C, const U128* __restrict__ H, U128* __restrict__ G) {
  using F = Fe<FP>;
  using W = Fe29<FP>;
  __shared__ int32_t lds[9 * SCAN_BLOCK_THREADS];   // [limb][thread]
  constexpr int K = SCAN_PER_THREAD;
  const uint32_t t = threadIdx.x, job = blockIdx.x;
  H += 2 * (size_t)job * SCAN_CHUNKS;
  G += 2 * (size_t)job * SCAN_CHUNKS;
  auto put = [&](uint32_t i, const W& x) {
#pragma unroll
    for (int l = 0; l < 9; l++) lds[l * SCAN_BLOCK_THREADS + i] = x.v[l];
  };
  auto get = [&](uint32_t i) {
    W x;
#pragma unroll
    for (int l = 0; l < 9; l++) x.v[l] = lds[l * SCAN_BLOCK_THREADS + i];
    return x;
  };
  const W one = fe29_from_api(F::one());
  const uint32_t T = (C + K - 1) / K;               // threads that hold values
  if (mode == 0) {
    // data scaled like the API's bytes (see above); y_c = sum_{j >= c} w^(j-c) v_j, G[c] = y_(c+1)
    W wk[K + 1];                                    // w^0 .. w^K, true working form, normalised
    wk[0] = one;
    wk[1] = fe29_mul(expr_column_operand(B.w[job]), one);
#pragma unroll
    for (int k = 2; k <= K; k++) wk[k] = fe29_mul(wk[k - 1], wk[1]);
    W s[K];
#pragma unroll
    for (int k = 0; k < K; k++) s[k] = t * K + k < C ? fe29_unpack(fe_load<FP>(H + 2 * (t * K + k))) : W::zero();
#pragma unroll
    for (int k = K - 2; k >= 0; k--) s[k] = fe29_norm(fe29_add(s[k], fe29_mul(wk[1], s[k + 1])));
    W y = s[0];                                     // the group's total, weights counted from its first chunk
    W wp = wk[K];
    for (uint32_t st = 1; st < T; st <<= 1) {
      put(t, y);
      __syncthreads();
      if (t + st < T) y = fe29_norm(fe29_add(y, fe29_mul(wp, get(t + st))));
      __syncthreads();
      wp = fe29_mul(wp, wp);
    }
    put(t, y);
    __syncthreads();
    const W next = t + 1 < T ? get(t + 1) : W::zero();    // y of the following group's first chunk
    // y_(tK+k) = s_k + w^(K-k) next; G[tK+k] = y_(tK+k+1), and G of the group's last chunk is `next`
#pragma unroll
    for (int k = 0; k < K; k++) {
      const uint32_t c = t * K + k;
      if (c >= C) break;
      const W v = k + 1 < K ? fe29_add(s[k + 1], fe29_mul(wk[K - k - 1], next)) : fe29_mul(next, one);
      fe_store<FP>(G + 2 * c, w_canonical_pack(k + 1 < K ? fe29_mul(fe29_norm(v), one) : v));
    }
  } else {
    // G[c] = prod_{j < c} v_j
    W p[K];
#pragma unroll
    for (int k = 0; k < K; k++) p[k] = t * K + k < C ? expr_column_operand(fe_load<FP>(H + 2 * (t * K + k))) : one;
    p[0] = fe29_mul(p[0], one);
#pragma unroll
    for (int k = 1; k < K; k++) p[k] = fe29_mul(p[k - 1], p[k]);
    W y = p[K - 1];
    for (uint32_t st = 1; st < T; st <<= 1) {
      put(t, y);
      __syncthreads();
      if (t >= st) y = fe29_mul(y, get(t - st));
      __syncthreads();
    }
    put(t, y);
    __syncthreads();
    const W before = t > 0 ? get(t - 1) : one;      // product of every group below this one
#pragma unroll
    for (int k = 0; k < K; k++) {
      const uint32_t c = t * K + k;
      if (c >= C) break;
      fe_store<FP>(G + 2 * c, fe29_to_api(k == 0 ? before : fe29_mul(before, p[k - 1])));
    }
  }
}
template <class FP>
__global__ void __launch_bounds__(64)
poly_scan_apply_kernel(ScanBatch<FP> B, int mode, size_t n, uint32_t L, uint32_t C, const U128* __restrict__ G) {
  using F = Fe<FP>;
  using W = Fe29<FP>;
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x, job = blockIdx.y;
  if (c >= C) return;
  const U128* a = B.a[job];
  U128* out = B.out[job];
  const size_t lo = (size_t)c * L, hi = min(n, lo + L);
  const U128* g = G + 2 * ((size_t)job * SCAN_CHUNKS + c);
  if (mode == 0) {
    W cur = fe29_unpack(fe_load<FP>(g));
    const W z = expr_column_operand(B.z[job]);
    for (size_t top = hi; top > lo;) {
      const uint32_t cnt = (uint32_t)min((size_t)SCAN_AHEAD, top - lo);
      F v[SCAN_AHEAD];
#pragma unroll
      for (int k = 0; k < SCAN_AHEAD; k++)
        if ((uint32_t)k < cnt) v[k] = fe_load<FP>(a + 2 * (top - 1 - k));
#pragma unroll
      for (int k = 0; k < SCAN_AHEAD; k++)
        if ((uint32_t)k < cnt) {
          const size_t i = top - 1 - k;
          cur = fe29_add(fe29_mul(cur, z), fe29_unpack(v[k]));
          if (i >= 1) fe_store<FP>(out + 2 * (i - 1), w_canonical_pack(cur));
        }
      top -= cnt;
    }
    if (c == C - 1) fe_store<FP>(out + 2 * (n - 1), F::zero());
  } else {
    W cur = fe29_mul(expr_column_operand(fe_load<FP>(g)), fe29_from_api(F::one()));
    for (size_t at = lo; at < hi;) {
      const uint32_t cnt = (uint32_t)min((size_t)SCAN_AHEAD, hi - at);
      F v[SCAN_AHEAD];
#pragma unroll
      for (int k = 0; k < SCAN_AHEAD; k++)
        if ((uint32_t)k < cnt) v[k] = fe_load<FP>(a + 2 * (at + k));
#pragma unroll
      for (int k = 0; k < SCAN_AHEAD; k++)
        if ((uint32_t)k < cnt) {
          fe_store<FP>(out + 2 * (at + k), fe29_to_api(cur));
          cur = fe29_mul(cur, expr_column_operand(v[k]));
        }
      at += cnt;
    }
  }
}

// ---- eval_polynomial: out[job] = sum_{i < n} poly_job[i] x_job^i, many (polynomial, point) jobs per launch sequence -------
// halo2_proofs @6b43b6b src/arithmetic.rs `eval_polynomial` (create_proof evaluates every advice, fixed, permutation and
// quotient polynomial at x w^rot before it opens them).  Three launches, every one deterministic, grid.y = job:
//   powers   one thread per job: x^R, x^2R, x^4R, ..., x^T by 4 + log2(threads) squarings -- the only powers the job needs,
//            computed once, so no thread exponentiates for itself
//   tile     a workgroup of POLY_EVAL_THREADS threads covers T = POLY_EVAL_TILE coefficients: each thread runs Horner over
//            its own R = POLY_EVAL_RUN consecutive coefficients (R - 1 products), then the workgroup folds its threads'
//            values pairwise, lo + x^(R 2^l) hi at level l, compacting through LDS so that level l keeps only
//            threads / 2^(l+1) lanes busy (whole waves drop out); one value per (job, tile) goes to HBM
//   fold     one thread per job: Horner over the job's tile values in x^T, the result in the API's form
// Products per job: about n (1 - 1/R) in the runs, n / R in the trees, 4 + log2(threads) for the powers, n / T in the fold.
// Scratch per job (POLY_EVAL_WS_BYTES): ceil(n / T) tile values of 32 bytes and POLY_EVAL_POWERS powers of 36 bytes.
//
// Magnitudes, in units of p, on the 9 x 29-bit lazy form (h2_field29.hpp; R' = 2^261 > 128 p for the three fields):
//   * a coefficient or point in HBM is x 2^256, canonical; expr_column_operand (shifted unpack minus 16 p) makes it the
//     working form of x in (-16 p, 16 p) with limbs below 2^29 in magnitude.  A slot past the end of the polynomial is
//     loaded as 0 and becomes -16 p: zero mod p, inside the same bounds, so runs and tiles need no special last case.
//   * a Horner step is acc' = acc x / R' + c.  fe29_mul asks for limbs below 2^30 on one side and below 2^29 on the other
//     and nothing of the values; it returns normalised limbs and a value in (a b / R' - p, a b / R'].  With |x| < 16 p a
//     product is below |acc| / 8 + p, so |acc| <= M + 16 p with M = (M + 16 p) / 8 + p, M = 24 p / 7: every acc stays below
//     20 p.  acc' is a normalised product plus a fresh operand: limbs below 2^29 + 2^29 = 2^30, a valid FIRST operand of
//     the next product as it is (no carry pass); the point, the second operand, keeps limbs below 2^29.
//   * the powers are products of normalised values below 1.2 p (x 1 / R' first, then squares): |pw| < 1.2 p.
//   * a tree level is lo + hi pw / R': below |lo| + |hi| / 100 + p, so each of the at most 10 levels adds less than
//     1.3 p to the 20 p of a run: below 33 p.  A level's result is the sum of two normalised values, limbs below 2^30;
//     it is carry-normalised before it goes to LDS, so both what a level reads are valid operands.
//   * a tile value leaves through fe29_to_api (any |x| < 64 p) as canonical API limbs; the fold reads them back through
//     expr_column_operand and is the same Horner step with x^T (|pw| < 1.2 p) for the point: below 20 p, out through
//     fe29_to_api -- canonical Montgomery limbs, bit-exact whatever the grouping.
constexpr int POLY_EVAL_RUN = 16;                                   // R: coefficients per thread
constexpr int POLY_EVAL_AHEAD = 4;                                  // coefficients loaded ahead of a run's chain
constexpr int POLY_EVAL_THREADS = 256;
constexpr int POLY_EVAL_TILE = POLY_EVAL_RUN * POLY_EVAL_THREADS;   // T = 4096 coefficients per workgroup
constexpr int POLY_EVAL_LEVELS = 8;                                 // log2(threads)
constexpr int POLY_EVAL_POWERS = POLY_EVAL_LEVELS + 1;              // x^(R 2^l), l = 0 .. log2(threads): the last is x^T
constexpr size_t POLY_EVAL_MAX_N = (size_t)1 << 30;
constexpr size_t POLY_EVAL_WS_CAP = (size_t)64 << 20;                // scratch of the jobs that share a launch sequence
static_assert((1 << POLY_EVAL_LEVELS) == POLY_EVAL_THREADS && (POLY_EVAL_RUN & (POLY_EVAL_RUN - 1)) == 0, "powers of two");
inline size_t poly_eval_tiles(size_t n) { return (n + POLY_EVAL_TILE - 1) / POLY_EVAL_TILE; }
// scratch of `jobs` jobs: the tile values (32-byte elements first, for their alignment), then the powers
inline size_t poly_eval_ws_bytes(size_t jobs, size_t n) { return jobs * (poly_eval_tiles(n) * 32 + POLY_EVAL_POWERS * 36); }

template <class FP>
__global__ void __launch_bounds__(64)
poly_eval_powers_kernel(const PolyEvalJob* __restrict__ jobs, uint32_t njobs, int32_t* __restrict__ powers) {
  using W = Fe29<FP>;
  const uint32_t job = blockIdx.x * blockDim.x + threadIdx.x;
  if (job >= njobs) return;
  Fe<FP> x;
#pragma unroll
  for (int i = 0; i < 8; i++) x.v[i] = jobs[job].point[i];
  W p = fe29_mul(expr_column_operand(x), fe29_from_api(Fe<FP>::one()));    // |p| < 16 p p / R' + p < 1.2 p
  for (int r = 1; r < POLY_EVAL_RUN; r <<= 1) p = fe29_sqr(p);              // x^R
  int32_t* dst = powers + (size_t)job * POLY_EVAL_POWERS * 9;
  for (int l = 0; l < POLY_EVAL_POWERS; l++) {
#pragma unroll
    for (int i = 0; i < 9; i++) dst[l * 9 + i] = p.v[i];
    p = fe29_sqr(p);
  }
}

template <class FP>
__global__ void __launch_bounds__(POLY_EVAL_THREADS)
poly_eval_tile_kernel(const PolyEvalJob* __restrict__ jobs, size_t n, const int32_t* __restrict__ powers,
                      U128* __restrict__ partial, uint32_t tiles) {
  using F = Fe<FP>;
  using W = Fe29<FP>;
  constexpr int R = POLY_EVAL_RUN, TH = POLY_EVAL_THREADS;
  __shared__ int32_t lds[2][9 * TH];                    // [buffer][limb][entry]: a level reads one, writes the other
  __shared__ int32_t pw[POLY_EVAL_LEVELS * 9];          // x^(R 2^l), l < log2(threads)
  const uint32_t t = threadIdx.x, tile = blockIdx.x, job = blockIdx.y;
  const PolyEvalJob& J = jobs[job];
  const U128* __restrict__ a = (const U128*)J.poly;
  const size_t base = (size_t)tile * POLY_EVAL_TILE;    // < n: the grid has ceil(n / T) tiles
  const size_t left = n - base;
  // entries of this tile that hold coefficients: the tree runs on these alone
  uint32_t cnt = left >= (size_t)POLY_EVAL_TILE ? (uint32_t)TH : (uint32_t)((left + R - 1) / R);
  int32_t my_pw = 0;
  if (t < POLY_EVAL_LEVELS * 9) my_pw = powers[(size_t)job * POLY_EVAL_POWERS * 9 + t];    // in flight during the run
  auto put = [&](int b, uint32_t i, const W& x) {
#pragma unroll
    for (int l = 0; l < 9; l++) lds[b][l * TH + i] = x.v[l];
  };
  auto get = [&](int b, uint32_t i) {
    W x;
#pragma unroll
    for (int l = 0; l < 9; l++) x.v[l] = lds[b][l * TH + i];
    return x;
  };
  W cur = W::zero();
  if (t < cnt) {
    const size_t lo = base + (size_t)t * R;
    F x;
#pragma unroll
    for (int i = 0; i < 8; i++) x.v[i] = J.point[i];
    const W xw = expr_column_operand(x);
    // from the run's top coefficient down, POLY_EVAL_AHEAD at a time; the next batch is loaded before this one's products
    // (the chain itself cannot hide a load).  The loop stays rolled: its body is four products, and a run unrolled whole
    // keeps R coefficients live at once
    constexpr int A = POLY_EVAL_AHEAD;
    auto load = [&](F* v, int top) {                    // coefficients top - 1 .. top - A of the run; 0 past the end
#pragma unroll
      for (int j = 0; j < A; j++) {
        const size_t i = lo + (size_t)(top - 1 - j);
        v[j] = i < n ? fe_load<FP>(a + 2 * i) : F::zero();
      }
    };
    F now[A], next[A];
    load(now, R);
    W acc = W::zero();
#pragma nounroll
    for (int top = R; top > 0; top -= A) {
      if (top > A) load(next, top - A);
#pragma unroll
      for (int j = 0; j < A; j++) {
        const W c = expr_column_operand(now[j]);
        acc = (j == 0 && top == R) ? c : fe29_add(fe29_mul(acc, xw), c);
      }
#pragma unroll
      for (int j = 0; j < A; j++) now[j] = next[j];
    }
    cur = fe29_norm(acc);
    put(0, t, cur);
  }
  if (t < POLY_EVAL_LEVELS * 9) pw[t] = my_pw;
  __syncthreads();
  int b = 0;
  for (int l = 0; cnt > 1; l++) {                       // cnt is the same for the whole workgroup
    const uint32_t half = (cnt + 1) >> 1;
    if (t < half) {
      cur = get(b, 2 * t);
      if (2 * t + 1 < cnt) {
        W p;
#pragma unroll
        for (int i = 0; i < 9; i++) p.v[i] = pw[l * 9 + i];
        cur = fe29_norm(fe29_add(cur, fe29_mul(get(b, 2 * t + 1), p)));
      }
      put(b ^ 1, t, cur);
    }
    __syncthreads();
    b ^= 1;
    cnt = half;
  }
  if (t == 0) fe_store<FP>(partial + 2 * ((size_t)job * tiles + tile), fe29_to_api(cur));
}

template <class FP>
__global__ void __launch_bounds__(64)
poly_eval_fold_kernel(uint32_t njobs, const int32_t* __restrict__ powers, const U128* __restrict__ partial, uint32_t tiles,
                      U128* __restrict__ out) {
  using W = Fe29<FP>;
  const uint32_t job = blockIdx.x * blockDim.x + threadIdx.x;
  if (job >= njobs) return;
  W y;                                                  // x^T
#pragma unroll
  for (int i = 0; i < 9; i++) y.v[i] = powers[((size_t)job * POLY_EVAL_POWERS + POLY_EVAL_LEVELS) * 9 + i];
  const U128* v = partial + 2 * (size_t)job * tiles;
  W acc = expr_column_operand(fe_load<FP>(v + 2 * (size_t)(tiles - 1)));
  for (uint32_t top = tiles - 1; top > 0;) {            // values loaded ahead of the chain, as in the scan kernels
    const uint32_t cnt = min((uint32_t)SCAN_AHEAD, top);
    Fe<FP> c[SCAN_AHEAD];
#pragma unroll
    for (int k = 0; k < SCAN_AHEAD; k++)
      if ((uint32_t)k < cnt) c[k] = fe_load<FP>(v + 2 * (size_t)(top - 1 - k));
#pragma unroll
    for (int k = 0; k < SCAN_AHEAD; k++)
      if ((uint32_t)k < cnt) acc = fe29_add(fe29_mul(acc, y), expr_column_operand(c[k]));
    top -= cnt;
  }
  fe_store<FP>(out + 2 * (size_t)job, fe29_to_api(acc));
}

// ---- linear combinations of resident columns: out_j[i] = sum_t c_t a_t[i] - low_j[i], grid.y = job -------------------------
// The column work of the multiopen argument (halo2_proofs @6b43b6b src/poly/kzg/multiopen/{gwc,shplonk}/prover.rs: the
// v-power sum of the polynomials opened at one point, the y-power sum of a rotation set minus its remainder, the final
// L(X)) and the join of the quotient pieces h(X) = sum x^(n i) h_i(X) in front of it (src/plonk/vanishing/prover.rs
// `Constructed::evaluate`).  One thread per row; jobs and terms come from tables in HBM (uniform per workgroup: scalar
// loads), so any number of terms is one launch.  The divisions that follow a sum are the scan kernels above, mode 0.
//
// On the 9 x 29-bit lazy form, the data never converted (as in the scan's mode 0): a column element in HBM is the integer
// d = x 2^256 mod p, plain-unpacked; the coefficient goes through expr_column_operand, the integer c' = c 2^261 + j p in
// (-16 p, 16 p); fe29_mul(d, c') = d c' / R' is x c 2^256 mod p, the API form of the term, in (-9p/8, p/8] with
// normalised limbs.  Magnitudes, in units of p (R' = 2^261 > 128 p):
//   * two terms are added to the normalised sum limb-wise (limbs below 3 * 2^29 < 2^31) and one carry pass follows;
//   * every POLY_LINCOMB_FOLD = 32 terms the sum is multiplied by the working form of one (2^261 mod p, canonical): the
//     value is unchanged mod p and falls below |acc| / 128 + p.  Between folds |acc| < 1.4 p + 32 * 9p/8 < 38 p: the top
//     limb stays below 38 * 2^23 < 2^29, a valid operand on either side;
//   * the low coefficient (canonical, plain-unpacked) is subtracted limb-wise: |acc| < 39 p, limbs below 2^29 in magnitude;
//   * the last product with one lands in (-39p/128 - p, 39p/128]: inside fe29_canonical_pack's (-2p, p).  One such product
//     per stored element; the stored limbs are canonical, so the bits do not depend on how jobs share launches.
// T + 1 products per element against T products, T canonical additions and T final subtractions of fe_add(fe_mul()).
constexpr int POLY_LINCOMB_THREADS = 256;
constexpr uint32_t POLY_LINCOMB_FOLD = 32;
constexpr size_t POLY_LINCOMB_MAX_N = (size_t)1 << 30;
constexpr int POLY_LINCOMB_MAX_ROUNDS = 8;                            // linear factors one job may divide out
constexpr size_t POLY_LINCOMB_WS_CAP = (size_t)256 << 20;             // intermediate columns of the jobs that share a group
static_assert(POLY_LINCOMB_FOLD % 2 == 0, "the fold follows a pair of terms");

template <class FP>
__global__ void __launch_bounds__(POLY_LINCOMB_THREADS)
poly_lincomb_kernel(const LincombJob* __restrict__ jobs, const LincombTerm* __restrict__ terms, const U128* __restrict__ low,
                    size_t n) {
  using F = Fe<FP>;
  using W = Fe29<FP>;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const LincombJob job = jobs[blockIdx.y];
  const LincombTerm* __restrict__ tt = terms + job.first_term;
  auto coeff = [&](uint32_t t) {
    F c;
#pragma unroll
    for (int l = 0; l < 8; l++) c.v[l] = tt[t].coeff[l];
    return expr_column_operand(c);
  };
  auto column = [&](uint32_t t) { return fe_load<FP>((const U128*)tt[t].poly + 2 * i); };
  const W one = fe29_from_api(F::one());
  W acc = W::zero();
  uint32_t t = 0;
  for (; t + 2 <= job.n_terms; t += 2) {
    const F x0 = column(t), x1 = column(t + 1);            // both loads in flight before the first product
    const W p0 = fe29_mul(fe29_unpack(x0), coeff(t));
    const W p1 = fe29_mul(fe29_unpack(x1), coeff(t + 1));
    acc = fe29_norm(fe29_add(fe29_add(acc, p0), p1));
    if ((t + 2) % POLY_LINCOMB_FOLD == 0) acc = fe29_mul(acc, one);
  }
  if (t < job.n_terms) acc = fe29_norm(fe29_add(acc, fe29_mul(fe29_unpack(column(t)), coeff(t))));
  if (i < job.n_low) acc = fe29_sub(acc, fe29_unpack(fe_load<FP>(low + 2 * ((size_t)job.first_low + i))));
  fe_store<FP>((U128*)job.out + 2 * i, fe29_canonical_pack(fe29_mul(acc, one)));
}

// ---- the blinding polynomial's coefficients ------------------------------------------------------------------
// out[i] = Scalar::random(ChaCha20Rng::from_seed(seed)) number first + i (halo2_proofs @6b43b6b
// src/plonk/vanishing/prover.rs `Argument::commit`: random_poly from a ChaCha20Rng seeded off the prover's rng;
// SURVEY.md App. A.4).  rand_chacha 0.3.1: 20 rounds, 64-bit block counter in words 12-13, stream id 0; ff's
// `random` reads one 64-byte block as a 512-bit little-endian integer and reduces it: lo R + hi 2^256 R, formed
// as two Montgomery products with R^2 and R^3.
struct ChaChaKey { uint32_t w[8]; };

__device__ __forceinline__ uint32_t chacha_rotl(uint32_t v, int c) { return (v << c) | (v >> (32 - c)); }
#define H2_CHACHA_QR(a, b, c, d)            \
  a += b; d = chacha_rotl(d ^ a, 16);       \
  c += d; b = chacha_rotl(b ^ c, 12);       \
  a += b; d = chacha_rotl(d ^ a, 8);        \
  c += d; b = chacha_rotl(b ^ c, 7)

// ff's from_bytes_wide / Challenge255: the 512-bit integer lo + hi 2^256 reduced, as Montgomery limbs.  lo, hi < 2^256 need
// not be reduced: a Montgomery product with one factor < p is < 2p before its final subtraction
template <class FP>
H2_HD Fe<FP> fe_from_wide(const Fe<FP>& lo, const Fe<FP>& hi) {
  Fe<FP> r2;
#pragma unroll
  for (int k = 0; k < 8; k++) r2.v[k] = FP::R2(k);
  const Fe<FP> r3 = fe_mul(r2, r2);
  return fe_add(fe_mul(lo, r2), fe_mul(hi, r3));
}

template <class FP>
__global__ void __launch_bounds__(256)
chacha20_scalars_kernel(U128* __restrict__ out, size_t n, uint64_t first_block, ChaChaKey key) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t ctr = first_block + i;
  uint32_t in[16] = {0x61707865u, 0x3320646Eu, 0x79622D32u, 0x6B206574u, key.w[0], key.w[1], key.w[2], key.w[3],
                     key.w[4], key.w[5], key.w[6], key.w[7], (uint32_t)ctr, (uint32_t)(ctr >> 32), 0u, 0u};
  uint32_t x0 = in[0], x1 = in[1], x2 = in[2], x3 = in[3], x4 = in[4], x5 = in[5], x6 = in[6], x7 = in[7],
           x8 = in[8], x9 = in[9], x10 = in[10], x11 = in[11], x12 = in[12], x13 = in[13], x14 = in[14], x15 = in[15];
  for (int r = 0; r < 10; r++) {
    H2_CHACHA_QR(x0, x4, x8, x12); H2_CHACHA_QR(x1, x5, x9, x13); H2_CHACHA_QR(x2, x6, x10, x14); H2_CHACHA_QR(x3, x7, x11, x15);
    H2_CHACHA_QR(x0, x5, x10, x15); H2_CHACHA_QR(x1, x6, x11, x12); H2_CHACHA_QR(x2, x7, x8, x13); H2_CHACHA_QR(x3, x4, x9, x14);
  }
  Fe<FP> lo, hi;
  lo.v[0] = x0 + in[0]; lo.v[1] = x1 + in[1]; lo.v[2] = x2 + in[2]; lo.v[3] = x3 + in[3];
  lo.v[4] = x4 + in[4]; lo.v[5] = x5 + in[5]; lo.v[6] = x6 + in[6]; lo.v[7] = x7 + in[7];
  hi.v[0] = x8 + in[8]; hi.v[1] = x9 + in[9]; hi.v[2] = x10 + in[10]; hi.v[3] = x11 + in[11];
  hi.v[4] = x12 + in[12]; hi.v[5] = x13 + in[13]; hi.v[6] = x14 + in[14]; hi.v[7] = x15 + in[15];
  fe_store<FP>(out + 2 * i, fe_from_wide(lo, hi));
}
#undef H2_CHACHA_QR

inline unsigned poly_grid(size_t total) {
  size_t b = (total + 255) / 256;
  if (b > 256 * 8) b = 256 * 8;  // 8 blocks per CU, grid-stride the rest
  if (b < 1) b = 1;
  return (unsigned)b;
}

}  // namespace h2
