// h2_prover_kernels.hpp -- device kernels of the C++ prover (h2_prover.hip), all over bn256::Fr.
//
// These are the pieces of halo2_proofs::plonk::create_proof that sit BETWEEN the MSM / NTT calls (SURVEY.md App. A.4,
// A.7; reached from /root/reference/circuits/src/utils.rs:83-91,105-120): witness columns, the permutation grand
// product, the quotient numerator, evaluations at the challenge point, the opening combinations.  prover.py runs
// them as ~600 generic pointwise launches; here each is ONE launch for every proof of a lockstep group (h2_prove.hpp):
//   * expr_kernel            the whole quotient numerator -- every gate, the permutation argument, the y-fold and the
//                            division by the vanishing polynomial -- as a straight-line program interpreted per row
//                            of the extended coset (operands: extended columns with rotations, constants, LDS slots);
//                            generic over the field, in h2_expr_kernel.hpp
//   * perm_ratio_kernel      prod (v + beta delta^j w^i + gamma) / prod (v + beta sigma_j + gamma) with one inversion
//                            per 4 rows (Montgomery's trick)
//   * poly_eval_kernels      all evaluations of the group (different polynomials at different points) in two launches
//   * lincomb_batch_kernel   out_j = sum_t c_t a_t for a list of jobs (lincomb_kernel, up to 24 columns of one sum by
//                            value, serves setup, keygen and the verifiers)
//   * coset_shrink           the zeta^-i scaling of the kept prefix after the inverse extended-domain NTT (the way in,
//                            zero-extension and zeta^i, is pass 0 of the extending NTT: h2_ntt29.hpp)
//   * scale_kernel, sub_prefix_kernel   a column times a constant; a remainder's low coefficients subtracted
// All HBM-bound elementwise work except expr_kernel (a few hundred field products per row).
// The prover's kernels take grid.y = job or proof and read what differs between jobs -- a handful of pointers and
// constants -- from a table in HBM: the prover uploads a phase's tables once (Proving::Steps), which makes one proof cost
// what arguments passed by value would, and N proofs one launch.  Field results are canonical, so a proof's bytes do
// not depend on how many jobs share its launches.
#pragma once
#include "h2_expr_kernel.hpp"
#include "h2_field.hpp"
#include "h2_field29.hpp"

namespace h2 {
namespace pk {

using FR = BN254_FR;
using F = Fe<FR>;

// ---- the 9 x 29-bit lazy form (h2_field29.hpp) for bn256::Fr in these kernels ---------------------------------------------
// A product is ~240 instructions there against ~600 on 8 x 32-bit limbs with carries, and a lone wave runs a chain of
// them about twice as fast -- most kernels below are chains (an inversion, a program's instructions).  HBM keeps the
// API's form x 2^256; a value goes in through expr_column_operand (shifted unpack minus 16 p, no product) and out
// through one product with 2^256 (fe29_to_api), which gives the canonical API bytes back.
using W = Fe29<FR>;
__device__ __forceinline__ W w_load(const U128* p) { return expr_column_operand(fe_load<FR>(p)); }
__device__ __forceinline__ W w_from(const F& a) { return expr_column_operand(a); }
__device__ __forceinline__ void w_store(U128* p, const W& x) { fe_store<FR>(p, fe29_to_api(x)); }
// a^(p-2), two exponent bits at a time (254 squarings + ~96 products; the exponent is a constant, the branches uniform)
__device__ __forceinline__ W w_inv(const W& a) {
  const W a2 = fe29_mul(a, a), a3 = fe29_mul(a2, a);
  uint32_t e[8];
#pragma unroll
  for (int i = 0; i < 8; i++) e[i] = FR::P(i);
  e[0] -= 2;                                  // bn256::Fr: p[0] = 0xf0000001, no borrow
  W r = fe29_from_api(F::one());
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

// column[cell.row] = cell.value for `count` cells (values in Montgomery form); the column was zero-filled before
struct CellRef {
  uint32_t col, row;
};
static __global__ void __launch_bounds__(256)
scatter_cells_kernel(U128* __restrict__ base, size_t col_stride /* elements */, const CellRef* __restrict__ refs,
                     const U128* __restrict__ vals, uint32_t count) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  U128* dst = base + 2 * ((size_t)refs[i].col * col_stride + refs[i].row);
  dst[0] = vals[2 * i];
  dst[1] = vals[2 * i + 1];
}

// grid.y = proof: out[p][i] = in[p][i] * zinv^i for i < count (after the inverse extended NTT) -- the n (d-1) kept
// coefficients of every proof's quotient, written compactly (out_stride = count) from the extended columns (in_stride = en)
static __global__ void __launch_bounds__(256)
coset_shrink_kernel(const U128* __restrict__ in, size_t in_stride, U128* __restrict__ out, size_t out_stride, uint32_t count,
                    F zi1, F zi2) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const U128* src = in + 2 * (in_stride * blockIdx.y + i);
  U128* dst = out + 2 * (out_stride * blockIdx.y + i);
  F v = fe_load<FR>(src);
  const uint32_t r = i % 3;
  if (r != 0) v = fe_mul(v, r == 1 ? zi1 : zi2);
  fe_store<FR>(dst, v);
}

// ---- permutation grand product: ratio[i] = prod_j (v_j + beta delta^j w^i + gamma) / prod_j (v_j + beta sigma_j + gamma)
constexpr int PERM_MAX_COLS = 8;
constexpr int PERM_RUN = 4;      // rows per thread: one inversion per run (Montgomery's trick)
struct PermArgs {
  const U128* value[PERM_MAX_COLS];
  const U128* sigma[PERM_MAX_COLS];
  F beta_delta[PERM_MAX_COLS];   // beta * delta^j
  F beta, gamma;
  int ncols;
};
// grid.y = (proof, set), one PermArgs per ratio column in HBM (the columns of a proof only share beta and gamma); ratio:
// one column per PermArgs; PERM_RUN rows per thread
static __global__ void __launch_bounds__(256)
perm_ratio_kernel(const PermArgs* __restrict__ args, const U128* __restrict__ omega_col, U128* __restrict__ ratio_base, uint32_t n) {
  const PermArgs& A = args[blockIdx.y];
  U128* __restrict__ ratio = ratio_base + 2 * (size_t)n * blockIdx.y;
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t lo = t * PERM_RUN;
  if (lo >= n) return;
  const W gamma = w_from(A.gamma), beta = w_from(A.beta);
  W num[PERM_RUN], den[PERM_RUN], pre[PERM_RUN];
  const W one = fe29_from_api(F::one());
  W acc = one;
  for (int k = 0; k < PERM_RUN; k++) {
    const uint32_t i = lo + k;
    W nu = one, de = one;
    if (i < n) {
      const W w = w_load(omega_col + 2 * (size_t)i);
      for (int j = 0; j < A.ncols; j++) {
        // v + gamma: three terms at most 16 p + p: normalised before it enters a product as the second operand
        const W vg = fe29_add(w_load(A.value[j] + 2 * (size_t)i), gamma);
        nu = fe29_mul(nu, fe29_norm(fe29_add(fe29_mul(w, w_from(A.beta_delta[j])), vg)));
        de = fe29_mul(de, fe29_norm(fe29_add(fe29_mul(w_load(A.sigma[j] + 2 * (size_t)i), beta), vg)));
      }
    }
    num[k] = nu;
    den[k] = de;
    pre[k] = acc;
    acc = fe29_mul(acc, de);
  }
  W inv = w_inv(acc);         // a zero denominator (probability 2^-250 per row) would zero the run, as 1/0 := 0 does
  for (int k = PERM_RUN - 1; k >= 0; k--) {
    const uint32_t i = lo + k;
    if (i < n) w_store(ratio + 2 * (size_t)i, fe29_mul(num[k], fe29_mul(pre[k], inv)));
    inv = fe29_mul(inv, den[k]);
  }
}
// grid.y = job: a[i] *= c for i < n
struct ScaleJob {
  U128* a;
  F c;
};
static __global__ void __launch_bounds__(256) scale_kernel(const ScaleJob* __restrict__ jobs, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const ScaleJob job = jobs[blockIdx.y];
  fe_store<FR>(job.a + 2 * (size_t)i, fe_mul(fe_load<FR>(job.a + 2 * (size_t)i), job.c));
}

// grid.y = job: a[i] -= v[offset + i] for i < count (the low coefficients of a remainder; `v` is one table for the launch)
struct SubPrefixJob {
  U128* a;
  uint32_t offset, count;
};
static __global__ void __launch_bounds__(64) sub_prefix_kernel(const SubPrefixJob* __restrict__ jobs, const U128* __restrict__ v) {
  const SubPrefixJob job = jobs[blockIdx.y];
  for (uint32_t i = threadIdx.x; i < job.count; i += blockDim.x)
    fe_store<FR>(job.a + 2 * (size_t)i,
                 fe_sub(fe_load<FR>(job.a + 2 * (size_t)i), fe_load<FR>(v + 2 * ((size_t)job.offset + i))));
}

// ---- out[i] = sum_j c_j a_j[i] ---------------------------------------------------------------------------------
constexpr int LINCOMB_MAX = 24;
struct LincombArgs {
  const U128* a[LINCOMB_MAX];
  F c[LINCOMB_MAX];
  int count;
  int unit_first;   // c[0] == 1: skip its product
};
static __global__ void __launch_bounds__(256)
lincomb_kernel(LincombArgs A, U128* __restrict__ out, uint32_t n, int accumulate) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  F acc = accumulate ? fe_load<FR>(out + 2 * (size_t)i) : F::zero();
  for (int j = 0; j < A.count; j++) {
    const F v = fe_load<FR>(A.a[j] + 2 * (size_t)i);
    acc = fe_add(acc, (j == 0 && A.unit_first) ? v : fe_mul(v, A.c[j]));
  }
  fe_store<FR>(out + 2 * (size_t)i, acc);
}

// grid.y = job: out[i] = sum_t c_t a_t[i] over the job's `count` terms, which start at terms[first].  `out` may be one
// of the job's own operands (the sum is elementwise)
struct LincombTerm {
  const U128* a;
  F c;
};
struct LincombJob {
  U128* out;
  uint32_t first, count;
};
static __global__ void __launch_bounds__(256)
lincomb_batch_kernel(const LincombJob* __restrict__ jobs, const LincombTerm* __restrict__ terms, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const LincombJob job = jobs[blockIdx.y];
  F acc = F::zero();
  for (uint32_t t = 0; t < job.count; t++) {
    const LincombTerm term = terms[job.first + t];
    acc = fe_add(acc, fe_mul(fe_load<FR>(term.a + 2 * (size_t)i), term.c));
  }
  fe_store<FR>(job.out + 2 * (size_t)i, acc);
}

// ---- evaluations: job q = (polynomial pointer, point); partial[q][block] then out[q] ------------------------------
constexpr int EVAL_RUN = 8;        // coefficients per thread
constexpr int EVAL_BLOCK = 256;
struct EvalJob {
  const U128* poly;
  F point;
};
static __global__ void __launch_bounds__(EVAL_BLOCK)
poly_eval_partial_kernel(const EvalJob* __restrict__ jobs, uint32_t n, U128* __restrict__ partial, uint32_t blocks_per_job) {
  __shared__ U128 red[2 * EVAL_BLOCK];
  const EvalJob job = jobs[blockIdx.y];
  const uint32_t t = blockIdx.x * EVAL_BLOCK + threadIdx.x;
  const uint32_t lo = t * EVAL_RUN;
  F acc = F::zero();
  if (lo < n) {
    const uint32_t hi = min(n, lo + EVAL_RUN);
    for (uint32_t i = hi; i-- > lo;) acc = fe_add(fe_mul(acc, job.point), fe_load<FR>(job.poly + 2 * (size_t)i));
    acc = fe_mul(acc, fe_pow_u64(job.point, lo));
  }
  fe_store<FR>(red + 2 * threadIdx.x, acc);
  __syncthreads();
  for (uint32_t s = EVAL_BLOCK / 2; s > 0; s >>= 1) {
    if (threadIdx.x < s)
      fe_store<FR>(red + 2 * threadIdx.x, fe_add(fe_load<FR>(red + 2 * threadIdx.x), fe_load<FR>(red + 2 * (threadIdx.x + s))));
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    U128* dst = partial + 2 * ((size_t)blockIdx.y * blocks_per_job + blockIdx.x);
    dst[0] = red[0];
    dst[1] = red[1];
  }
}
static __global__ void __launch_bounds__(64)
poly_eval_final_kernel(const U128* __restrict__ partial, uint32_t blocks_per_job, U128* __restrict__ out, uint32_t njobs) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= njobs) return;
  F acc = F::zero();
  for (uint32_t b = 0; b < blocks_per_job; b++) acc = fe_add(acc, fe_load<FR>(partial + 2 * ((size_t)q * blocks_per_job + b)));
  fe_store<FR>(out + 2 * (size_t)q, acc);
}

// ---- the quotient numerator as a straight-line program: XInstr, the EXPR_* constants and expr_kernel, generic over the
// scalar field, are in h2_expr_kernel.hpp; the prover launches the bn256::Fr instantiation through CurveOps::expr_launch

}  // namespace pk
}  // namespace h2
