// h2_prover_kernels.hpp -- device kernels of the C++ prover (h2_prover.hip), all over bn256::Fr.
//
// These are the pieces of halo2_proofs::plonk::create_proof that sit BETWEEN the MSM / NTT calls (SURVEY.md App. A.4,
// A.7; reached from /root/reference/circuits/src/utils.rs:83-91,105-120): witness columns, the permutation grand
// product, the quotient numerator, evaluations at the challenge point, the opening combinations.  prover.py runs
// them as ~600 generic pointwise launches; here each is ONE launch for every proof of a lockstep group (h2_prove.hpp):
//   * expr_kernel            the whole quotient numerator -- every gate, the permutation argument, the y-fold and the
//                            division by the vanishing polynomial -- as a straight-line program interpreted per row
//                            of the extended coset (operands: extended columns with rotations, constants, LDS slots)
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

// ---- the quotient numerator as a straight-line program -----------------------------------------------------------------
// operand word: bits 31..30 = kind (0 slot, 1 constant, 2 column, 3 the previous instruction's result); slot / constant:
// index in bits 29..0; column: index in bits 29..8, rotation + 128 in bits 7..0.
// op_dst: op in bits 31..24 (0 add, 1 sub, 2 mul), slot in 23..0 (X_NO_STORE: only the next instruction reads it).
struct XInstr {
  uint32_t op_dst, a, b;
};
constexpr uint32_t X_SLOT = 0u << 30, X_CONST = 1u << 30, X_COL = 2u << 30, X_PREV = 3u << 30;
constexpr uint32_t X_NO_STORE = 0xFFFFFFu;     // destination field of a result that only the next instruction reads
constexpr int EXPR_BLOCK = 64;
constexpr int EXPR_REG_SLOTS = 4;       // slots kept in registers (expr_kernel); the rest is LDS
constexpr size_t EXPR_LDS_MAX = 160 * 1024;   // dynamic LDS one workgroup may hold (expr_kernel has no static LDS)
// magnitudes, in units of p, that the host's compiler (ExprProgram::compile) assumes: a column operand after
// expr_column_operand, and the largest value an instruction may produce before it is reduced by a product with one
constexpr int EXPR_COLUMN_BOUND = 16, EXPR_VALUE_BOUND = 32;

// The arithmetic runs on the 9 x 29-bit lazy form (h2_field29.hpp: for bn256::Fr a product is ~240 instructions
// against ~600 on 8 x 32-bit limbs with carries):
//   * a column holds x 2^256 (canonical); shifted left by five bits while it is unpacked that is the integer
//     x 2^261 + (a multiple of p) < 32 p, the working form of x -- minus 16 p it lies in (-16 p, 16 p);
//   * the constant table is uploaded in the working form (c 2^261 mod p, canonical) and only unpacked;
//   * sums and differences are carry-normalised, products need nothing; the compiler keeps every value that is stored
//     or forwarded below EXPR_VALUE_BOUND p (it multiplies a sum by one where it would exceed that bound: the sum, at
//     most 2 EXPR_VALUE_BOUND p, is then that product's operand).  fe29_mul needs only its limb bounds, which every
//     normalised value of magnitude below 2^260 meets; a product of two such values, up to (32 p)^2 = 1024 p^2, is
//     past the 64 p^2 that gives fe29_mul's (-3p/2, p/2] range, and lies in (a b / R' - p, a b / R'], |x| < 9 p;
//     fe29_to_api takes any |x| < 64 p;
//   * the last result goes back to the API form (one product) on its way out.
// Operands that do not depend on the program's own results -- columns and constants -- are fetched TWO instructions
// ahead (a global load is 0.5-2 us, an instruction 0.1-0.5).  LDS: 36 bytes per slot beyond the register slots and row.
// grid.y = proof.  One program and one set of row masks; proof p reads its column pointers at cols + p ncols, its
// constants (y, beta, gamma, beta delta^j differ) at consts + p nconsts and writes the extended column out + p en
static __global__ void __launch_bounds__(EXPR_BLOCK)
expr_kernel(const XInstr* __restrict__ prog, uint32_t ninstr, const U128* const* __restrict__ all_cols, uint32_t ncols,
            const uint32_t* __restrict__ col_mask, const U128* __restrict__ all_consts, uint32_t nconsts,
            U128* __restrict__ all_out, uint32_t step, uint32_t en) {
  const U128* const* __restrict__ cols = all_cols + (size_t)blockIdx.y * ncols;
  const U128* __restrict__ consts = all_consts + 2 * (size_t)blockIdx.y * nconsts;
  U128* __restrict__ out = all_out + 2 * (size_t)blockIdx.y * en;
  using W = Fe29<FR>;
  extern __shared__ int32_t slots[];      // [slot][limb][thread]
  const uint32_t tid = threadIdx.x;
  const uint32_t i = blockIdx.x * EXPR_BLOCK + tid;
  // slots 0 .. EXPR_REG_SLOTS-1 live in registers: the slot number comes from the instruction word, the same for the
  // whole wave, so the choice is a scalar branch around nine moves -- nothing next to a 240-instruction product, and
  // the LDS that is left (Poseidon: 3 slots instead of 7) no longer caps the waves per SIMD
  W reg0 = W::zero(), reg1 = W::zero(), reg2 = W::zero(), reg3 = W::zero();
  auto slot_load = [&](uint32_t s) {
    if (s == 0) return reg0;
    if (s == 1) return reg1;
    if (s == 2) return reg2;
    if (s == 3) return reg3;
    W r;
#pragma unroll
    for (int l = 0; l < 9; l++) r.v[l] = slots[((s - EXPR_REG_SLOTS) * 9 + l) * EXPR_BLOCK + tid];
    return r;
  };
  // a column or constant operand as loaded (a slot operand is read when its instruction runs)
  auto fetch = [&](uint32_t code) -> F {
    const uint32_t kind = code & (3u << 30);
    if (kind == X_SLOT || kind == X_PREV) return F::zero();
    if (kind == X_CONST) return fe_load<FR>(consts + 2 * (size_t)(code & 0x3FFFFFFFu));
    const uint32_t c = (code >> 8) & 0x3FFFFFu;
    const int rot = (int)(code & 0xFFu) - 128;
    const uint32_t idx = (i + (uint32_t)(rot * (int)step)) & col_mask[c];
    return fe_load<FR>(cols[c] + 2 * (size_t)idx);
  };
  const XInstr nop{0u, X_SLOT, X_SLOT};
  auto instr_at = [&](uint32_t k) { return k < ninstr ? prog[k] : nop; };
  W r = W::zero();
  auto operand = [&](uint32_t code, const F& pre) -> W {
    const uint32_t kind = code & (3u << 30);
    if (kind == X_SLOT) return slot_load(code & 0x3FFFFFFFu);
    if (kind == X_PREV) return r;
    if (kind == X_CONST) return fe29_unpack(pre);
    return expr_column_operand(pre);
  };
  // one instruction: operands from the prefetched pair, the register or LDS; the pair is refilled for instruction k + 2
  // (the instruction words travel the same way: `ins` was read two instructions ago and is replaced by the one two ahead)
  auto run = [&](uint32_t k, XInstr& slot_ins, F& pa, F& pb) {
    const XInstr ins = slot_ins;
    const W a = operand(ins.a, pa), b = operand(ins.b, pb);
    const XInstr ahead = instr_at(k + 2);
    slot_ins = ahead;
    pa = fetch(ahead.a);
    pb = fetch(ahead.b);
    const uint32_t op = ins.op_dst >> 24;
    if (op == 2) r = fe29_mul(a, b);
    else r = fe29_norm(op == 0 ? fe29_add(a, b) : fe29_sub(a, b));
    const uint32_t s = ins.op_dst & 0xFFFFFFu;
    if (s == 0) reg0 = r;
    else if (s == 1) reg1 = r;
    else if (s == 2) reg2 = r;
    else if (s == 3) reg3 = r;
    else if (s != X_NO_STORE) {
#pragma unroll
      for (int l = 0; l < 9; l++) slots[((s - EXPR_REG_SLOTS) * 9 + l) * EXPR_BLOCK + tid] = r.v[l];
    }
  };
  XInstr i0 = instr_at(0), i1 = instr_at(1);
  F pa0 = fetch(i0.a), pb0 = fetch(i0.b), pa1 = fetch(i1.a), pb1 = fetch(i1.b);
  for (uint32_t k = 0; k < ninstr; k += 2) {
    run(k, i0, pa0, pb0);
    if (k + 1 < ninstr) run(k + 1, i1, pa1, pb1);
  }
  if (i < en) fe_store<FR>(out + 2 * (size_t)i, fe29_to_api(r));     // a domain smaller than one block: the spare lanes computed on wrapped rows
}

}  // namespace pk
}  // namespace h2
