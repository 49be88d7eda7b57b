// h2_curve_ops.hpp -- per-curve launch table.  Each curve's kernels are compiled in their own
// translation unit (h2_curve_impl.hip with -DH2_CURVE_ID=0/1/2) so the three build in parallel;
// h2_capi.hip holds only host logic and calls through this table.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace h2 {

struct U128;
struct MsmGeom;
struct MsmWorkspace;
struct LookupWorkspace;
struct PermWorkspace;
struct IpaOne;

// one evaluation: the polynomial's coefficients in HBM (API form, 16-byte aligned) and the point's 8 x 32-bit
// Montgomery limbs.  The poly_eval kernels read a table of these from HBM (h2_poly.hpp)
struct PolyEvalJob {
  const void* poly;
  uint32_t point[8];
};

// one term and one job of poly_lincomb (h2_poly.hpp), laid out as h2_lincomb_term_t / h2_lincomb_job_t of the C ABI: the
// column in HBM (API form, 16-byte aligned) and its coefficient's 8 x 32-bit Montgomery limbs; the job's output and its
// ranges in the term table and the table of low coefficients (the kernel does not read the points)
struct LincombTerm {
  const void* poly;
  uint32_t coeff[8];
};
struct LincombJob {
  void* out;
  uint32_t first_term, n_terms, first_low, n_low, first_point, n_points;
};
static_assert(sizeof(LincombTerm) == 40 && sizeof(LincombJob) == 32, "the C ABI's layout");

struct CurveOps {
  int curve_id;
  int scalar_field_id;
  uint32_t scalar_bits;
  // raise the dynamic-LDS limits of this curve's kernels on the current device (once per device, from h2_init)
  hipError_t (*kernel_setup)();
  // MSM
  // d_bad: device counter (zeroed by the caller) of points that are not on the curve
  // d_scratch: MSM_TABLE_SCRATCH (80) bytes per window and point
  hipError_t (*table_build)(const void* d_bases, void* d_table, void* d_scratch, uint32_t n, const MsmGeom& g, uint32_t* d_bad, hipStream_t s);
  hipError_t (*msm_launch)(const void* d_table, const void* const* per_column_tables, uint32_t n_bases, const void* d_scalars, size_t n, size_t col_stride, size_t m,
                           const MsmGeom& g, char* ws_base, const MsmWorkspace& ws, hipStream_t s,
                           hipEvent_t ev_start, hipEvent_t ev_stop, hipEvent_t ev_tail,
                           void* d_out_jac /* optional: m Jacobian results, written by the MSM's last kernel */,
                           bool zeroed /* the workspace's zeroed region is zero already (left so by the previous launch sequence) */);
  // table-free MSM over points passed with the call (h2_msm_points.hpp): g = msm_points_geometry, ws = msm_points_workspace,
  // both proven by msm_points_check; m Jacobian results
  hipError_t (*msm_points_launch)(const void* d_points_affine, const void* d_scalars, size_t n, size_t col_stride, size_t m,
                                  const MsmGeom& g, char* ws_base, const MsmWorkspace& ws, hipStream_t s, void* d_out_jac,
                                  bool zeroed);
  hipError_t (*srs_powers)(void* d_out_affine, const uint64_t s_mont[4], uint32_t n, hipStream_t s);
  hipError_t (*fixed_base_mul)(void* d_out_affine, const void* d_scalars, uint32_t n, hipStream_t s);
  // `count` <= MSM_SMALL_MAX independent MSMs of a few dozen arbitrary points each (no table), side by side:
  // d_work = count * (ceil(max m / 16) * 144 bytes) and count 4-byte counters behind them (zeroed here);
  // count Jacobian points out
  hipError_t (*msm_small)(const void* const* d_points_affine, const void* const* d_scalars, const uint32_t* m, uint32_t count,
                          void* d_work, void* d_out_jac, hipStream_t s);
  hipError_t (*to_affine)(const void* d_xyzz, void* d_out, uint32_t m, hipStream_t s);
  // d_out[j] = sum_g d_in[g * count + j], Jacobian points in the API form
  hipError_t (*points_sum)(const void* d_in_jac, void* d_out_jac, uint32_t groups, uint32_t count, hipStream_t s);
  // n compressed points (32 bytes each, the transcript's wire form) -> n affine points in the API form and n status
  // bytes (h2_decompress.hpp); NULL for curves whose base field has no square root by a single power (Pallas, Vesta)
  hipError_t (*points_decompress)(const void* d_compressed, void* d_out_affine, void* d_status, uint32_t n, hipStream_t s);
  // the same routine instantiated on the host, one point per call (CPU tests); NULL where points_decompress is
  int (*selftest_decompress)(const uint8_t in[32], uint64_t out_affine[8]);
  // square roots in the base field (h2_sqrt.hpp), every curve: n elements in the API form -> n even roots and n status bytes;
  // d_out may be d_in
  hipError_t (*base_sqrt)(const void* d_in, void* d_out, void* d_status, uint32_t n, hipStream_t s);
  // points_decompress for the Pasta wire form (bit 255 the parity, no identity flag; h2_decompress.hpp); NULL for BN254
  hipError_t (*pasta_points_decompress)(const void* d_compressed, void* d_out_affine, void* d_status, uint32_t n, hipStream_t s);
  // the same two routines instantiated on the host, one element or point per call (CPU tests); the second NULL for BN254
  int (*selftest_base_sqrt)(const uint64_t in_mont[4], uint64_t out_mont[4]);
  int (*selftest_pasta_decompress)(const uint8_t in[32], uint64_t out_affine[8]);
  // NTT over the scalar field
  // the tables of one (omega, log n [, constant]): inter-pass twiddles, unpacked radix twiddles per pass, the
  // canonicalisation table (h2_ntt29.hpp).  ntt_scale_in_table: a transform scaled by a constant takes that constant
  // from tables built with it (two-pass plans); otherwise the final pass multiplies
  size_t (*ntt_table_bytes)(uint32_t log_n);
  bool (*ntt_scale_in_table)(uint32_t log_n);
  hipError_t (*ntt_twiddles)(void* d_tables, const uint64_t omega[4], uint32_t log_n, hipStream_t s, const uint64_t* scale /* or null */);
  hipError_t (*ntt_launch)(void* d_data, void* d_scratch, const void* d_tw, uint32_t log_n, size_t m,
                           hipStream_t s, const uint64_t* scale /* 4 limbs or null */);
  // coeff_to_extended: m columns of 2^log_src coefficients (src_stride elements apart, read only) -> m columns of
  // 2^log_n values in d_out: the transform of the zero-extended column times zeta^i, the padding never materialised
  // (pass 0 of h2_ntt29.hpp's extending kernel).  Tables of (omega, log_n) unscaled; log_n >= 1; d_scratch as ntt_launch
  hipError_t (*ntt_extend_launch)(const void* d_src, size_t src_stride, uint32_t log_src, const uint64_t zeta[4], void* d_out,
                                  void* d_scratch, const void* d_tw, uint32_t log_n, size_t m, hipStream_t s);
  // extended_to_coeff (with divide_by_vanishing_poly when d_t is set): m columns of 2^log_n values (read only) ->
  // out[c][j] = zi[j mod 3] scale sum_i src[c][i] t[i mod t_period] w^(ij) for j < out_len, columns out_stride apart,
  // nothing written beyond out_len (the dividing pass 0 and the shrinking final pass of h2_ntt29.hpp).  Tables of
  // (w, log_n), built with `scale` when ntt_scale_in_table(log_n); none needed for log_n = 0; d_scratch as ntt_launch
  hipError_t (*ntt_coeff_launch)(const void* d_src, const void* d_t, size_t t_period, const uint64_t scale[4],
                                 const uint64_t zeta_inv[4], void* d_out, size_t out_len, size_t out_stride, void* d_scratch,
                                 const void* d_tw, uint32_t log_n, size_t m, hipStream_t s);
  // best_fft over group elements (FftGroup for the curve: g_to_lagrange): n = 2^log_n Jacobian points (API form) in,
  // the transform out (may alias), natural order, unscaled; d_scratch: group_fft_scratch(log_n) bytes.
  // lanes: 0 = the stage kernel's form by size, 1 or 4 = that form (h2_selftest_set_gfft_lanes)
  size_t (*group_fft_scratch)(uint32_t log_n);
  hipError_t (*group_fft)(const void* d_in_jac, void* d_out_jac, void* d_scratch, const uint64_t omega[4], uint32_t log_n,
                          int lanes, hipStream_t s);
  // ParamsKZG's g_to_lagrange on that transform: n affine points in (identity (0, 0)), out[i] = [scale] sum_j
  // [omega^(ij)] in[j] normalised (may alias); same scratch
  hipError_t (*g_to_lagrange)(const void* d_in_affine, void* d_out_affine, void* d_scratch, const uint64_t omega[4],
                              const uint64_t scale[4], uint32_t log_n, int lanes, hipStream_t s);
  // host: the GLV split of a canonical scalar of this curve's scalar field as the kernels take it (h2_selftest_glv_split)
  void (*selftest_glv_split)(const uint64_t k_canonical[4], uint32_t out[10]);
  // host: lambda (canonical, scalar field) and beta (Montgomery, base field) of the split's endomorphism
  void (*selftest_glv_constants)(uint64_t lambda[4], uint64_t beta[4]);
  int glv_bits;     // GLV_BITS: both magnitudes of a split are below 2^glv_bits
  // pointwise polynomial kernels over the scalar field (EvaluationDomain pieces)
  hipError_t (*poly_scale)(void* d_a, size_t total, const uint64_t c[4], hipStream_t s);
  hipError_t (*poly_powers)(void* d_a, size_t n, size_t m, const uint64_t g[4], hipStream_t s);
  hipError_t (*poly_mul_periodic)(void* d_a, size_t total, const void* d_t, size_t period, hipStream_t s);
  hipError_t (*poly_pointwise)(void* d_a, const void* d_b, size_t total, int op, hipStream_t s);
  hipError_t (*poly_inverse)(void* d_a, size_t total, hipStream_t s);
  // 1 <= jobs <= SCAN_MAX_JOBS (8) scans of n >= 1 elements side by side (h2_poly.hpp); d_ws: jobs * SCAN_WS_BYTES
  // (2 * 4096 * 32) bytes.  mode 0: d_out[j] = (d_a[j] - d_a[j](z_j)) / (X - z_j), z: 4 limbs per job, d_out[j] != d_a[j];
  // mode 1: d_out[j][i] = prod_{t < i} d_a[j][t] (d_out[j][0] = 1; may alias d_a[j]), z unused
  hipError_t (*poly_scan)(int mode, const void* const* d_a, void* const* d_out, const uint64_t* z, uint32_t jobs, size_t n,
                          void* d_ws, hipStream_t s);
  // d_out[t] = sum_{i < n} poly_t[i] point_t^i for the 1 <= jobs <= 65535 entries of the table d_jobs (grid.y = job),
  // 1 <= n <= 2^30 coefficients each; d_ws: poly_eval_ws_bytes(jobs, n), 16-byte aligned (h2_poly.hpp); three launches
  hipError_t (*poly_eval)(const PolyEvalJob* d_jobs, uint32_t jobs, size_t n, void* d_ws, void* d_out, hipStream_t s);
  // out_j[i] = sum_t coeff_t poly_t[i] - (i < n_low_j ? d_low[first_low_j + i] : 0) for i < n and the 1 <= jobs <= 65535
  // entries of the table d_jobs (grid.y = job), their terms in the table d_terms; 1 <= n <= 2^30; one launch
  hipError_t (*poly_lincomb)(const LincombJob* d_jobs, uint32_t jobs, const LincombTerm* d_terms, const void* d_low, size_t n,
                             hipStream_t s);
  // permute_expression_pair of ws.mm lookups of ws.u rows (h2_lookup.hpp): inputs and tables col_stride elements apart, ws
  // proven by lookup_check, ws_base its scratch; d_status (ws.mm words) zeroed by the caller
  hipError_t (*lookup_permute)(const void* d_input, const void* d_table, size_t col_stride, const LookupWorkspace& ws, char* ws_base,
                               void* d_permuted_input, void* d_permuted_table, uint32_t* d_status, hipStream_t s);
  // commit_product's per-row ratio into rows [0, u) of the m columns of d_z, row u = 1 (m <= 65535: grid.y)
  hipError_t (*lookup_ratio)(const void* d_input, const void* d_table, const void* d_permuted_input, const void* d_permuted_table,
                             size_t u, size_t col_stride, size_t m, const uint64_t beta[4], const uint64_t gamma[4], void* d_z,
                             hipStream_t s);
  // the permutation argument's grand products (h2_permutation.hpp); w proven by perm_check, base its scratch with the tables
  // uploaded.  perm_ratio: the ratios of `count` <= 65535 instances from p0 on into rows [0, u) of their S z columns, row u = 1
  hipError_t (*perm_ratio)(const PermWorkspace& w, char* base, size_t p0, size_t count, size_t u, size_t n_cols, size_t chunk_len,
                           size_t S, const uint64_t omega[4], void* d_z, size_t col_stride, hipStream_t s);
  // perm_scan: the running product of `count` <= 256 instances from p0 on, each over its S u ratios in (set, row) order, in
  // place; the value at every set boundary also lands in row u of the set before, the total in row u of the last.  S u > 0
  hipError_t (*perm_scan)(const PermWorkspace& w, char* base, size_t p0, size_t count, size_t u, size_t S, void* d_z, size_t col_stride,
                          hipStream_t s);
  // expr_kernel (h2_expr_kernel.hpp) over the scalar field: the compiled program d_code (ninstr x 12 bytes) on `rows` rows
  // of 1 <= count <= 65535 instances (grid.y).  Instance p: column pointers d_cols[p ncols ...], constants in the working
  // form d_consts + 32 (p nconsts), result at d_out + 32 (p out_stride).  d_masks: length - 1 of each column;
  // lds_bytes = expr_lds_for_slots of the program's slots, at most EXPR_LDS_MAX
  hipError_t (*expr_launch)(const void* d_code, uint32_t ninstr, const void* const* d_cols, uint32_t ncols, const uint32_t* d_masks,
                            const void* d_consts, uint32_t nconsts, void* d_out, size_t out_stride, uint32_t step, uint32_t rows,
                            uint32_t count, size_t lds_bytes, hipStream_t s);
  // d_out[i] = Scalar::random of ChaCha20 block first_block + i (key = the 32 seed bytes as 8 little-endian words)
  hipError_t (*chacha20_scalars)(void* d_out, size_t n, uint64_t first_block, const uint32_t key[8], hipStream_t s);
  // the inner product argument on the registered generators (h2_ipa.hpp): m <= IPA_MAX_BATCH openings of one k <= IPA_MAX_K
  // in lockstep, a single opening being m = 1; d_state: IpaBatchLayout(k, m).total elements.  The call's scalars: for
  // m >= 2 the state's table, already filled by a copy enqueued on s; for m = 1 `one`.  One launch of each kernel serves all
  // m.  ipa_begin: a_i = the 2^k coefficients d_p[i], b_i = the powers of x3_i, s_i = [1].  ipa_round: for j > 0 the fold by
  // u_prev, then the 2 m columns of 2^k + 2 scalars (the caller runs the MSM on them).  ipa_final: the last fold, d_out =
  // m x (c_i || b_i[0]), d_s_out (optional) = m x the finished s in natural order
  hipError_t (*ipa_begin)(uint32_t k, size_t m, const IpaOne& one, void* d_state, hipStream_t s);
  hipError_t (*ipa_round)(uint32_t k, uint32_t j, size_t m, const IpaOne& one, void* d_state, hipStream_t s);
  hipError_t (*ipa_final)(uint32_t k, size_t m, const IpaOne& one, void* d_state, void* d_out, void* d_s_out, hipStream_t s);
  // ipa_s_products: compute_s(u, init), u: k x 4 limbs on the host
  hipError_t (*ipa_s_products)(const uint64_t* u, uint32_t k, const uint64_t init[4], void* d_out, hipStream_t s);
  // the sum of `count` <= IPA_SUM_GROUP compute_s vectors from the table ipa_sum_fill made of them (d_table, in HBM), added
  // to what d_out holds when `accumulate`
  hipError_t (*ipa_s_sum)(const void* d_table, uint32_t count, uint32_t k, void* d_out, bool accumulate, hipStream_t s);
  // the IPA batch verifier's kernels (h2_ipa_verify.hpp).  ipa_replay: the transcripts of `count` proofs, one lane each
  // (h2_ipa_replay_device's arguments); NULL for BN254, whose wire form the batch verifier does not take.
  // ipa_verify_prepare: the replay's rows, x3, v and count x 8 words of weights -> the points MSM's scalar column, the sum
  // kernel's table and count x 3 terms.  ipa_verify_finish: d_col[0] -= the first terms' sum, rows 2^k and 2^k + 1 = minus
  // the other two
  hipError_t (*ipa_replay)(uint32_t k, size_t count, const void* d_states, const void* d_points, const void* d_point_status,
                           const void* d_scalars, void* d_out, void* d_status, void* d_states_out, hipStream_t s);
  hipError_t (*ipa_verify_prepare)(const void* d_replay, const void* d_x3, const void* d_v, const void* d_weights, void* d_scal,
                                   void* d_table, void* d_terms, uint32_t k, size_t count, hipStream_t s);
  hipError_t (*ipa_verify_finish)(const void* d_terms, size_t count, void* d_col, uint32_t k, hipStream_t s);
  // the IPA prover's transcript step (h2_ipa_prove.hpp), one lane per opening: behind round j < k of a state laid out by
  // IpaProveLayout(k, m) it writes L_j, R_j into the m proofs of d_tail, absorbs them, squeezes u_j and writes the scalar
  // table for the next round; j == k, behind the final kernel: c and f, the midstates into d_states_out (or null).
  // inv_form: 0 divsteps, 1 fe_inv (the comparison).  NULL for BN254, whose wire form it does not write
  hipError_t (*ipa_prove_step)(uint32_t k, uint32_t j, size_t m, void* d_state, void* d_tail, void* d_states_out, void* d_status,
                               int inv_form, hipStream_t s);
  // host self-test hooks (host instantiation of the same templates)
  int (*selftest_field)(int which /* 0 = base field, 1 = scalar field */, int op, const uint64_t* a,
                        const uint64_t* b, uint64_t* out);
  int (*selftest_curve)(int op, const uint64_t* p, const uint64_t* q, uint64_t* out);
  // the same field ops run by a device kernel on n element pairs (device pointers)
  hipError_t (*selftest_field_device)(int which, int op, const void* d_a, const void* d_b, void* d_out, uint32_t n,
                                      hipStream_t s);
  // the working-form group law on the device, four lanes per pair (op 0/1: quad add / double, 2/3: lane add /
  // double, 5: [k]p by the weight kernel's double-and-add with a different k per quad)
  hipError_t (*selftest_curve_device)(int op, const void* d_p, const void* d_q, void* d_out, uint32_t n, hipStream_t s);
  int (*selftest_digits)(const uint64_t* scalar_mont, size_t n_for_geometry, uint32_t* out, uint32_t cap);
  // dependent working-form products of the base field on `blocks` x 256 threads: measured modmul/s (best of 3)
  hipError_t (*modmul_rate)(int blocks, int iters, hipStream_t s, double* modmul_per_s);
  // the working-form group law on raw operands (h2_selftest_xyzz29_op*): in = two stored XYZZ points of 36 limbs, out = the
  // result's 36 limbs.  Host: ops 0..3.  Device: n pairs, four lanes per pair, each lane stores its own copy (n x 4 x 36
  // limbs); ops 4 / 5 the quad forms, 6 / 7 the affine forms on Fe29Chain (a form of its own only where base_chain29)
  bool base_chain29;
  int (*selftest_xyzz29)(int op, const int32_t* in, int32_t* out);
  hipError_t (*selftest_xyzz29_device)(int op, const void* d_in, void* d_out, uint32_t n, hipStream_t s);
};

const CurveOps* curve_ops_bn254();
const CurveOps* curve_ops_pallas();
const CurveOps* curve_ops_vesta();

}  // namespace h2
