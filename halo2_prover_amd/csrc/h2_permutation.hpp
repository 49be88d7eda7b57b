// h2_permutation.hpp -- the permutation argument's grand products over resident columns, generic over the field:
// halo2_proofs @6b43b6b src/plonk/permutation/prover.rs `Argument::commit`.  With u usable rows and the n_cols permutation
// columns cut into S sets of chunk_len,
//   ratio_s[i] = prod_{j in set s} (v_j[i] + beta delta^j omega^i + gamma) / prod_{j in set s} (v_j[i] + beta sigma_j[i] + gamma)
//   z_0[0] = 1,  z_s[i+1] = z_s[i] ratio_s[i] (i < u),  z_{s+1}[0] = z_s[u]
// Set s + 1 starts where set s ended, so the S columns of one instance are ONE running product over the sequence
// (set, row): a single scan that walks the sets in order carries last_z across them, and no tail ever goes to the host.
// Four launches whatever S and n_cols are:
//   perm_ratio_kernel        grid (tiles, S, instances): the ratios into rows [0, u) of every z column, 1 into row u
//   perm_scan_chunk_kernel   the product of every chunk of L >= 16 elements of an instance's S u ratios
//   poly_scan_block_kernel   (h2_poly.hpp, mode 1, as it is) the exclusive scan of an instance's <= SCAN_CHUNKS chunk values
//   perm_scan_apply_kernel   the recurrence inside every chunk, in place; the value at a set boundary also goes to row u of
//                            the set before, the total to row u of the last set
// Element e of an instance's sequence lives in column e / u at row e % u; row u of a column holds no ratio, so the scan
// may run in place.  All arithmetic is on the 9 x 29-bit working form (h2_field29.hpp): columns come in through
// expr_column_operand and leave through fe29_to_api, canonical Montgomery limbs -- the same bits whatever the grouping,
// the run length or the way omega^i is formed.
//
// Magnitudes in the ratio kernel, in units of p (R' = 2^261 > 128 p; fe29_mul returns a value in (a b / R' - p, a b / R']
// with normalised limbs for operands with limbs below 2^30 and 2^29):
//   * an operand from HBM or from the tables (value, sigma, beta, gamma, beta delta^j, a power of omega) is in (-16 p, 16 p),
//     limbs below 2^29 in magnitude;
//   * omega^i is a product of such operands started from 1: |w'| < |w| 16 / 128 + 1, so |w| < 1.2 p, normalised;
//   * a numerator term is w (beta delta^j) / R' + v + gamma: below 0.2 p + 1 p + 32 p; a denominator term is
//     sigma beta / R' + v + gamma: below 2 p + 1 p + 32 p = 35 p.  Three summands: carry-normalised (fe29_norm), then limbs
//     are below 2^29 (35 p < 2^261) and the term is a valid second operand;
//   * num and den start from 1 and take one term per column: |x'| < |x| 35 / 128 + 1, so below 1.4 p -- inside
//     fe29_is_zero_mod_p's |x| < 16 p and fe29_inv's "a product's result";
//   * the run's products, the inverse and the ratio are products of values below 1.4 p: below 1.1 p, out through
//     fe29_to_api (|x| < 64 p).
#pragma once
#include <type_traits>

#include "h2_curve_ops.hpp"
#include "h2_field.hpp"
#include "h2_field29.hpp"
#include "h2_poly.hpp"
#include "h2_tune.hpp"

namespace h2 {

constexpr int PERM_THREADS = 256;
constexpr int PERM_RUN = 4;                              // rows per thread: one Fermat inversion per run (Montgomery's trick)
// the run length in use: PERM_RUN, except in a tuning build (h2_tune.hpp), where H2_PERM_RUN may ask for 8 or 16
inline int perm_run() {
  const int r = tune_int("H2_PERM_RUN", PERM_RUN);
  return r == 8 || r == 16 ? r : PERM_RUN;
}
inline size_t perm_tile() { return (size_t)PERM_THREADS * perm_run(); }      // rows per workgroup
constexpr size_t PERM_MAX_ROWS = (size_t)1 << 26;
constexpr size_t PERM_MAX_CELLS = (size_t)1 << 57;       // m S col_stride
// powers of omega the host prepares: omega^(run 2^b), b < PERM_POW_BITS.  Thread g of a launch starts at row
// run g <= PERM_MAX_ROWS, so g < 2^PERM_POW_BITS
constexpr int PERM_POW_BITS = 25;
static_assert(((size_t)PERM_RUN << (PERM_POW_BITS - 1)) >= PERM_MAX_ROWS && (PERM_RUN & (PERM_RUN - 1)) == 0, "the power table covers every run");
constexpr size_t PERM_SCAN_GROUP = 256;                  // instances per scan launch sequence: 64 MiB of chunk values
constexpr size_t PERM_RATIO_GROUP = 65535;               // instances per ratio launch (grid.z)
constexpr size_t PERM_MAX_SETS = 65535;                  // grid.y

// what one (instance, column) contributes, read from a table in HBM: [p * n_cols + j]
struct PermColumn {
  const void* value;
  const void* sigma;
  uint32_t beta_delta[8];    // beta_p delta^j, Montgomery limbs
};
// per instance: [p]
struct PermChallenge {
  uint32_t beta[8], gamma[8];
};
static_assert(sizeof(PermColumn) == 48 && sizeof(PermChallenge) == 64, "table layouts");

// the call's scratch: the tables first (uploaded once), then the scan values of one group of instances
struct PermWorkspace {
  size_t off_columns, off_challenges, off_powers, off_scan, total;
  uint32_t tiles;            // ratio workgroups per column
  uint32_t L, C;             // scan: C chunks of L elements per instance
  size_t N;                  // S u: elements of an instance's sequence
};
inline PermWorkspace perm_workspace(size_t u, size_t n_cols, size_t S, size_t m, size_t scan_group) {
  PermWorkspace w{};
  size_t at = 0;
  auto take = [&](size_t bytes) {
    const size_t o = at;
    at += (bytes + 255) & ~(size_t)255;
    return o;
  };
  w.off_columns = take(m * n_cols * sizeof(PermColumn));
  w.off_challenges = take(m * sizeof(PermChallenge));
  w.off_powers = take(PERM_POW_BITS * 32);
  w.off_scan = take(scan_group * SCAN_WS_BYTES);
  w.total = at;
  w.tiles = (uint32_t)((u + 1 + perm_tile() - 1) / perm_tile());
  w.N = S * u;
  size_t L = (w.N + SCAN_CHUNKS - 1) / SCAN_CHUNKS;
  if (L < 16) L = 16;
  w.L = (uint32_t)L;
  w.C = (uint32_t)((w.N + L - 1) / L);
  return w;
}
// Every bound the kernels index by, proven on the host before anything is enqueued: the violated condition, or null
inline const char* perm_check(const PermWorkspace& w, size_t u, size_t n_cols, size_t chunk_len, size_t S, size_t m, size_t scan_group,
                              size_t col_stride, size_t arena_bytes) {
  if (u > PERM_MAX_ROWS) return "usable_rows <= 2^26";
  if (chunk_len == 0 || S != (n_cols + chunk_len - 1) / chunk_len) return "S == ceil(n_cols / chunk_len)";
  if (S == 0 || S > PERM_MAX_SETS) return "1 <= S <= 65535 (grid.y of the ratio kernel)";
  if (n_cols > ((size_t)1 << 31)) return "n_cols <= 2^31";
  if (col_stride < u + 1) return "col_stride >= usable_rows + 1";
  if (m == 0 || col_stride > PERM_MAX_CELLS / S / m) return "m S col_stride <= 2^57";
  if ((size_t)w.tiles * perm_tile() < u + 1) return "the ratio tiles cover rows [0, u]";
  if ((size_t)w.tiles * PERM_THREADS > ((size_t)1 << PERM_POW_BITS)) return "the power table covers every ratio thread";
  if (w.N != S * u) return "N == S u";
  if (w.N > 0 && (w.L < 16 || w.C == 0 || w.C > SCAN_CHUNKS || (size_t)w.L * w.C < w.N || (size_t)w.L * (w.C - 1) >= w.N))
    return "the scan's C <= 4096 chunks of L >= 16 elements cover the S u ratios exactly";
  if (scan_group == 0 || scan_group > PERM_SCAN_GROUP) return "1 <= instances per scan group <= 256";
  if (w.off_columns & 15 || w.off_challenges & 15 || w.off_powers & 15 || w.off_scan & 15) return "scratch offsets are 16-byte aligned";
  if (w.off_challenges < w.off_columns + m * n_cols * sizeof(PermColumn) || w.off_powers < w.off_challenges + m * sizeof(PermChallenge) ||
      w.off_scan < w.off_powers + PERM_POW_BITS * 32 || w.total < w.off_scan + scan_group * SCAN_WS_BYTES)
    return "the scratch regions do not overlap";
  if (w.total > arena_bytes) return "the scratch fits the arena";
  return nullptr;
}

struct PermRatioArgs {
  const PermColumn* columns;        // [(p0 + z) * n_cols + j]
  const PermChallenge* challenges;  // [p0 + z]
  const U128* powers;               // omega^(run 2^b), API form
  U128* z;                          // column (p0 + z) * S + y at z + 2 * col_stride * that
  size_t col_stride;
  uint32_t omega[8];
  uint32_t u, n_cols, chunk_len, S;
};

// f(0), ..., f(K - 1) with the index a compile-time constant: the per-row arrays of a run are then registers (a loop of
// products under `#pragma unroll` is past the compiler's size limit for unrolling and leaves them in scratch)
template <int K, class Fn>
__device__ __forceinline__ void perm_each(Fn&& f) {
  if constexpr (K > 0) {
    perm_each<K - 1>(f);
    f(std::integral_constant<int, K - 1>{});
  }
}

template <class FP>
__device__ __forceinline__ Fe29<FP> perm_operand(const uint32_t* limbs) {
  Fe<FP> x;
#pragma unroll
  for (int i = 0; i < 8; i++) x.v[i] = limbs[i];
  return expr_column_operand(x);
}

// grid (tiles, S, instances).  A thread owns RUN consecutive rows of one z column: the ratios of the rows below u by
// one shared inversion, a 1 at row u, nothing beyond.  A zero denominator is replaced by (num, den) = (0, 1): its row's
// ratio is 0 (batch_invert leaves zero at zero) and the inversion never sees a zero.
template <class FP, int RUN>
__global__ void __launch_bounds__(PERM_THREADS) perm_ratio_kernel(PermRatioArgs A, size_t p0) {
  using F = Fe<FP>;
  using W = Fe29<FP>;
  const uint32_t g = blockIdx.x * PERM_THREADS + threadIdx.x, u = A.u;
  const uint32_t lo = g * RUN;                      // < 2^27: the tiles end less than one tile past row u <= 2^26
  if (lo > u) return;
  const size_t p = p0 + blockIdx.z;
  const uint32_t s = blockIdx.y;
  const uint32_t j0 = s * A.chunk_len, j1 = min(A.n_cols, j0 + A.chunk_len);       // s < S: j0 < n_cols
  const PermColumn* __restrict__ cols = A.columns + p * A.n_cols;
  U128* __restrict__ z = A.z + 2 * A.col_stride * (p * A.S + s);
  const W one = fe29_from_api(F::one());
  const W beta = perm_operand<FP>(A.challenges[p].beta), gamma = perm_operand<FP>(A.challenges[p].gamma);
  const W omega = perm_operand<FP>(A.omega);
  // omega^lo = prod over the set bits b of g of omega^(RUN 2^b); g < 2^PERM_POW_BITS by perm_check
  W w = one;
  for (uint32_t b = 0, rest = g; rest; b++, rest >>= 1)
    if (rest & 1) w = fe29_mul(w, expr_column_operand(fe_load<FP>(A.powers + 2 * b)));
  // the columns outermost: a column's pointers and beta delta^j are read once per thread, its RUN rows loaded together
  W wk[RUN], num[RUN], den[RUN], pre[RUN];
  perm_each<RUN>([&](auto kc) {
    constexpr int k = decltype(kc)::value;
    wk[k] = w;
    num[k] = den[k] = one;
    if (k + 1 < RUN) w = fe29_mul(w, omega);
  });
  for (uint32_t j = j0; j < j1; j++) {
    const U128* __restrict__ value = (const U128*)cols[j].value;
    const U128* __restrict__ sigma = (const U128*)cols[j].sigma;
    const W bd = perm_operand<FP>(cols[j].beta_delta);
    perm_each<RUN>([&](auto kc) {
      constexpr int k = decltype(kc)::value;
      const uint32_t i = lo + k;
      if (i < u) {
        const W vg = fe29_add(expr_column_operand(fe_load<FP>(value + 2 * (size_t)i)), gamma);
        const W sg = expr_column_operand(fe_load<FP>(sigma + 2 * (size_t)i));
        num[k] = fe29_mul(num[k], fe29_norm(fe29_add(fe29_mul(wk[k], bd), vg)));
        den[k] = fe29_mul(den[k], fe29_norm(fe29_add(fe29_mul(sg, beta), vg)));
      }
    });
  }
  W acc = one;
  perm_each<RUN>([&](auto kc) {
    constexpr int k = decltype(kc)::value;
    if (fe29_is_zero_mod_p(den[k])) {
      num[k] = W::zero();
      den[k] = one;
    }
    pre[k] = acc;
    acc = fe29_mul(acc, den[k]);
  });
  W inv = fe29_inv(acc);
  perm_each<RUN>([&](auto kc) {
    constexpr int k = RUN - 1 - decltype(kc)::value;               // from the run's last row down
    const uint32_t i = lo + k;
    if (i < u) fe_store<FP>(z + 2 * (size_t)i, fe29_to_api(fe29_mul(num[k], fe29_mul(pre[k], inv))));
    else if (i == u) fe_store<FP>(z + 2 * (size_t)i, F::one());
    if (k > 0) inv = fe29_mul(inv, den[k]);
  });
}

// ---- the chained scan: h2_poly.hpp's three launches (mode 1) with element e of job p at column p S + e / u, row e % u --------
struct PermScanArgs {
  U128* z;                   // of the group's first instance
  size_t col_stride, N;      // N = S u > 0
  uint32_t u, S, L, C;
};

// the product of chunk c of instance blockIdx.y -> H[job][c]
template <class FP>
__global__ void __launch_bounds__(64) perm_scan_chunk_kernel(PermScanArgs A, U128* __restrict__ H) {
  using F = Fe<FP>;
  using W = Fe29<FP>;
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x, job = blockIdx.y;
  if (c >= A.C) return;
  const size_t lo = (size_t)c * A.L, hi = min(A.N, lo + A.L);          // lo < N: perm_check
  const U128* __restrict__ col = A.z + 2 * A.col_stride * ((size_t)job * A.S + lo / A.u);
  uint32_t row = (uint32_t)(lo % A.u);
  W acc = fe29_from_api(F::one());
  for (size_t at = lo; at < hi;) {
    const uint32_t cnt = (uint32_t)min((size_t)SCAN_AHEAD, hi - at);
    F v[SCAN_AHEAD];
#pragma unroll
    for (int k = 0; k < SCAN_AHEAD; k++)
      if ((uint32_t)k < cnt) {
        v[k] = fe_load<FP>(col + 2 * (size_t)row);
        if (++row == A.u) {                              // the next element is row 0 of the next set's column
          row = 0;
          col += 2 * A.col_stride;
        }
      }
#pragma unroll
    for (int k = 0; k < SCAN_AHEAD; k++)
      if ((uint32_t)k < cnt) acc = fe29_mul(acc, expr_column_operand(v[k]));
    at += cnt;
  }
  fe_store<FP>(H + 2 * ((size_t)job * SCAN_CHUNKS + c), fe29_to_api(acc));
}

// z[e] = G[c] prod of the chunk's elements below e, in place (an element is loaded before its slot is written).  The
// value at row 0 of set s > 0 is also the tail z_{s-1}[u]; the value after the last element is z_{S-1}[u].
template <class FP>
__global__ void __launch_bounds__(64) perm_scan_apply_kernel(PermScanArgs A, const U128* __restrict__ G) {
  using F = Fe<FP>;
  using W = Fe29<FP>;
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x, job = blockIdx.y;
  if (c >= A.C) return;
  const size_t lo = (size_t)c * A.L, hi = min(A.N, lo + A.L);
  uint32_t set = (uint32_t)(lo / A.u), row = (uint32_t)(lo % A.u);
  uint32_t wset = set, wrow = row;                       // where the value in hand is written: it trails the loads
  U128* __restrict__ first = A.z + 2 * A.col_stride * ((size_t)job * A.S);
  W cur = fe29_mul(expr_column_operand(fe_load<FP>(G + 2 * ((size_t)job * SCAN_CHUNKS + c))), fe29_from_api(F::one()));
  for (size_t at = lo; at < hi;) {
    const uint32_t cnt = (uint32_t)min((size_t)SCAN_AHEAD, hi - at);
    F v[SCAN_AHEAD];
#pragma unroll
    for (int k = 0; k < SCAN_AHEAD; k++)
      if ((uint32_t)k < cnt) {
        v[k] = fe_load<FP>(first + 2 * (A.col_stride * set + row));
        if (++row == A.u) {
          row = 0;
          set++;
        }
      }
#pragma unroll
    for (int k = 0; k < SCAN_AHEAD; k++)
      if ((uint32_t)k < cnt) {
        const F out = fe29_to_api(cur);
        fe_store<FP>(first + 2 * (A.col_stride * wset + wrow), out);
        if (wrow == 0 && wset > 0) fe_store<FP>(first + 2 * (A.col_stride * (wset - 1) + A.u), out);
        cur = fe29_mul(cur, expr_column_operand(v[k]));
        if (++wrow == A.u) {
          wrow = 0;
          wset++;
        }
      }
    at += cnt;
  }
  if (hi == A.N) fe_store<FP>(first + 2 * (A.col_stride * (A.S - 1) + A.u), fe29_to_api(cur));
}

// the ratios of instances [p0, p0 + count), count <= PERM_RATIO_GROUP; w proven by perm_check
template <class FP>
hipError_t perm_ratio_launch(const PermWorkspace& w, char* base, size_t p0, size_t count, size_t u, size_t n_cols, size_t chunk_len, size_t S,
                             const uint64_t omega[4], void* d_z, size_t col_stride, hipStream_t s) {
  PermRatioArgs A{};
  A.columns = (const PermColumn*)(base + w.off_columns);
  A.challenges = (const PermChallenge*)(base + w.off_challenges);
  A.powers = (const U128*)(base + w.off_powers);
  A.z = (U128*)d_z;
  A.col_stride = col_stride;
  memcpy(A.omega, omega, 32);
  A.u = (uint32_t)u;
  A.n_cols = (uint32_t)n_cols;
  A.chunk_len = (uint32_t)std::min<size_t>(chunk_len, n_cols);         // a longer chunk is one set of n_cols
  A.S = (uint32_t)S;
  const dim3 grid(w.tiles, (unsigned)S, (unsigned)count);
  switch (perm_run()) {
#ifdef H2_TUNING
    case 8: hipLaunchKernelGGL((perm_ratio_kernel<FP, 8>), grid, dim3(PERM_THREADS), 0, s, A, p0); break;
    case 16: hipLaunchKernelGGL((perm_ratio_kernel<FP, 16>), grid, dim3(PERM_THREADS), 0, s, A, p0); break;
#endif
    default: hipLaunchKernelGGL((perm_ratio_kernel<FP, PERM_RUN>), grid, dim3(PERM_THREADS), 0, s, A, p0);
  }
  return hipGetLastError();
}

// the chained scan of instances [p0, p0 + count), count <= PERM_SCAN_GROUP, N > 0
template <class FP>
hipError_t perm_scan_launch(const PermWorkspace& w, char* base, size_t p0, size_t count, size_t u, size_t S, void* d_z, size_t col_stride,
                            hipStream_t s) {
  PermScanArgs A{};
  A.z = (U128*)d_z + 2 * col_stride * (p0 * S);
  A.col_stride = col_stride;
  A.N = w.N;
  A.u = (uint32_t)u;
  A.S = (uint32_t)S;
  A.L = w.L;
  A.C = w.C;
  U128* H = (U128*)(base + w.off_scan);
  U128* G = H + 2 * count * SCAN_CHUNKS;
  const dim3 grid((w.C + 63) / 64, (unsigned)count);
  hipLaunchKernelGGL(perm_scan_chunk_kernel<FP>, grid, dim3(64), 0, s, A, H);
  hipLaunchKernelGGL(poly_scan_block_kernel<FP>, dim3((unsigned)count), dim3(SCAN_BLOCK_THREADS), 0, s, ScanBatch<FP>{}, 1, w.C, (const U128*)H, G);
  hipLaunchKernelGGL(perm_scan_apply_kernel<FP>, grid, dim3(64), 0, s, A, (const U128*)G);
  return hipGetLastError();
}

}  // namespace h2
