// h2_prover_kernels.hpp -- the C++ prover's own device kernels (h2_prove.hpp, h2_keygen.hpp, the verifiers), all over bn256::Fr.
//
// What is left of halo2_proofs::plonk::create_proof BETWEEN the shared calls -- the MSM, the transforms, the quotient
// program (h2_expr_kernel.hpp), the permutation grand products (h2_permutation.hpp), the evaluations and the scans
// (h2_poly.hpp), which the prover reaches through the *_enqueue functions of h2_internal.hpp as the C ABI does:
//   * scatter_cells_kernel   a sparse witness into zero-filled columns
//   * lincomb_batch_kernel   out_j = sum_t c_t a_t for a list of jobs (lincomb_kernel, up to 24 columns of one sum by
//                            value, serves setup, keygen and the verifiers)
//   * scale_kernel, sub_prefix_kernel   a column times a constant; a remainder's low coefficients subtracted
// All HBM-bound elementwise work on 8 x 32-bit Montgomery limbs, the API's form.
// The batch kernels take grid.y = job and read what differs between jobs -- a handful of pointers and constants -- from
// a table in HBM: the prover uploads a phase's tables once (Proving::Steps), which makes one proof cost what arguments
// passed by value would, and N proofs one launch.  Field results are canonical, so a proof's bytes do not depend on how
// many jobs share its launches.
#pragma once
#include "h2_field.hpp"

namespace h2 {
namespace pk {

using FR = BN254_FR;
using F = Fe<FR>;

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

}  // namespace pk
}  // namespace h2
