/*
 * h2hip_selftest.h -- host-side self-test hooks of libh2hip.so (not part of the drop-in ABI).
 *
 * The field / curve templates in halo2_prover_amd/csrc are __host__ __device__; these entry
 * points run the HOST instantiation of exactly that source so that `pytest -m "not gpu"` can
 * compare it with the CPU oracle on a machine without a GPU.  They are not a compute path:
 * one element per call, no batching, never used by the library itself.
 */
#ifndef H2HIP_SELFTEST_H
#define H2HIP_SELFTEST_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
/* field: 0 bn254_fq, 1 bn254_fr, 2 pasta_fp, 3 pasta_fq; op: 0 add, 1 sub, 2 mul, 3 inv, 4 to_mont,
 * 5 from_mont, 6 neg.  Operands / result: 4 x u64 Montgomery limbs. */
int h2_selftest_field_op(int field, int op, const uint64_t a[4], const uint64_t b[4], uint64_t out[4]);
/* curve ops on the host instantiation of the XYZZ formulas.  op: 0 = affine p + affine q,
 * 1 = 2 * affine p, 2 = (p + q) + q via xyzz_add of two accumulators, 3 = [k] p (k < 2^32, in q[0])
 * by double-and-add.  p, q: affine (8 limbs); out: affine (8 limbs), identity = zeros. */
int h2_selftest_curve_op(int curve, int op, const uint64_t p[8], const uint64_t q[8], uint64_t out[8]);
/* The same field ops through the DEVICE instantiation (gfx950 Comba multiplier): n element pairs, host
 * pointers, one kernel launch.  op 7 = the portable CIOS product compiled for the device (cross-check),
 * op 9 = the product through the MSM's 29-bit working form. */
int h2_selftest_field_op_device(int field, int op, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n);
/* the MSM's working-form group law (csrc/h2_curve29.hpp, h2_curve_quad.hpp) run by a device kernel on n pairs of
 * affine points (host pointers, 64 bytes each, API form; out: affine), four lanes per pair.  op 0 / 1: the
 * 4-lanes-per-point addition / doubling, 2 / 3: the one-lane forms, 4: double then add, 5: [k]p with k = the low
 * 32 bits of q.x by the weight kernel's double-and-add (a different k per quad: divergent control flow). */
int h2_selftest_curve_op_device(int curve, int op, const uint64_t* p, const uint64_t* q, uint64_t* out, size_t n);
/* host run of the signed-digit window decomposition used by the MSM digits kernel.
 * scalar: Montgomery limbs; geometry chosen as for `n_for_geometry` registered bases.
 * out[0..3] = widest window c, windows W, buckets B, scalar bits; out[4 + w] = 0 or |d| | sign << 31;
 * out[4 + W + w] = first bit of window w; out[4 + 2W + w] = width of window w (cap >= 4 + 3W).
 * Returns 0, or a negative value (cap too small / carry out of the top window). */
int h2_selftest_digits(int curve, const uint64_t scalar[4], size_t n_for_geometry, uint32_t* out, uint32_t cap);
/* test hook: cap the entries one sort launch may hold, so that the grouped-columns path of wide batches is reached
 * at small sizes; 0 restores the default (2^31 - 1). */
int h2_selftest_set_msm_max_entries(uint64_t limit);
/* MSM workspace checks.
 * h2_selftest_msm_check: host only, no GPU -- lays out the scratch arena of a launch of m columns of n scalars
 *   (col_stride elements apart) against n_bases registered bases and runs the bounds proof msm_device_run runs before
 *   every launch (each kernel's largest index against the region it indexes).  out[0..7] = window bits, windows,
 *   buckets, scalars per sort tile, staged scatter?, two-level sort?, entries per accumulate thread, regions.
 * h2_selftest_msm_front: host only -- the same layout and proof for the sort front of that launch (`pack` = 0: with the
 *   unpacked forms of h2_selftest_msm_guard(3)).  out[0..7] = scalars per sort tile, staged scatter?, its dynamic LDS in
 *   bytes, packed staged entries?, bits of a packed entry's bucket, index-in-tile and window fields, 1 if the bounds
 *   proof held; out[8..11] = entries per accumulate thread when every digit of the launch is non-zero (fewer entries
 *   never give more), the pieces above which a bucket takes the hot-task path, the pieces per hot task, the task slots.
 * h2_selftest_msm_fixup: host only -- the fix-up kernel's share of that layout (of the first launch, where the m columns
 *   take several).  out[0..3] = log2 of the lanes per key F,
 *   lanes of the launch (keys * F, without the task blocks), pieces per key the rule assumed, entries per accumulate thread.
 * h2_selftest_msm_tiles: host only -- the one-level sort's block -> (column, tile) mapping is a bijection onto the
 *   live pairs and every surplus block of the rounded-up grid is dead.
 * h2_selftest_msm_guard(1): from now on every MSM launch lays its arena out with a 256-byte red zone behind every
 *   region, fills the arena with a pattern first and counts the red-zone bytes that changed afterwards (synchronous;
 *   tests only; guard(2) also writes one byte behind the second region itself, to test the checker; guard(3) also makes
 *   the two-level sort carry the key's low bits in its side array, the layout of SRS sizes whose entries have no spare bits,
 *   and the staged scatter keep a reference and a 16-bit bucket per entry, the layout of geometries whose fields do not
 *   fit one word).
 *   h2_selftest_msm_guard_report: out[0] = launches checked, out[1] = regions overrun since guard(1);
 *   `first` = a description of the first one. */
int h2_selftest_msm_check(int curve, size_t n_bases, size_t n, size_t m, size_t col_stride, int guard, uint64_t out[8]);
int h2_selftest_msm_front(int curve, size_t n_bases, size_t n, size_t m, int pack, uint64_t out[12]);
int h2_selftest_msm_fixup(int curve, size_t n_bases, size_t n, size_t m, uint64_t out[4]);
int h2_selftest_msm_tiles(uint32_t tiles, uint32_t m);
int h2_selftest_msm_guard(int on);
int h2_selftest_msm_guard_report(uint64_t out[2], char* first, size_t cap);
/* The table-free MSM (h2_msm_points*).
 * h2_selftest_msm_points_check: host only, no GPU -- lays out the scratch arena of the bucket route for m columns of n
 *   scalars col_stride elements apart (the first column group, if m takes several) and runs the bounds proof that runs
 *   before every such launch sequence: msm_check's conditions for the m * W virtual columns behind the sort front, and the
 *   front's own (packed points, tile bases and group counters for m * W columns, the W * B histogram against the LDS, the
 *   31-bit entry).  out[0..7] = window bits, windows, buckets, scalars per sort tile, histogram bytes, columns in the
 *   group, entries per accumulate thread, regions.  H2_EINVAL for col_stride < n; H2_EDEVICE if a condition fails.
 *   h2_selftest_msm_guard(1) lays out and inspects these launch sequences' arenas as well.
 * h2_selftest_set_msm_points_small_max: tests only -- inputs of fewer than n terms take the double-and-add route; 0: every
 *   input takes buckets; SIZE_MAX restores the default (h2_msm_points_plan_t.crossover shows the value in force). */
int h2_selftest_msm_points_check(int curve, size_t n, size_t m, size_t col_stride, int guard, uint64_t out[8]);
int h2_selftest_set_msm_points_small_max(size_t n);
/* The group FFT (h2_fft_group*, h2_g_to_lagrange*; csrc/h2_group_fft.hpp).
 * h2_selftest_set_gfft_lanes: tests and tools only -- lanes per butterfly of the stage kernel: 1 or 4 forces that form at
 *   every size, 0 restores the choice by size (GFFT_QUAD_MAX_LOG_N).  H2_EINVAL for any other value.
 * h2_selftest_glv_split: host only, no GPU -- the host instantiation of the routine the twiddle kernel runs: the
 *   CANONICAL scalar k (4 x u64, below 2^256) of `curve`'s scalar field -> out[0..4] = |k1|, out[5..9] = |k2| as 32-bit words,
 *   least significant first, bit 31 of out[4] / out[9] set when k1 / k2 is negative; k1 + k2 lambda = k (mod r).
 * h2_selftest_glv_constants: host only -- lambda (canonical integer, scalar field), beta (Montgomery limbs, base field)
 *   with (beta x, y) = [lambda](x, y), and GLV_BITS, the loop length: both magnitudes are below 2^GLV_BITS. */
int h2_selftest_set_gfft_lanes(int lanes);
int h2_selftest_glv_split(int curve, const uint64_t k[4], uint32_t out[10]);
int h2_selftest_glv_constants(int curve, uint64_t lambda[4], uint64_t beta[4], uint32_t* glv_bits);
/* the integer ceiling the MSM kernels are priced against: dependent products of the MSM's working field form
 * (9 x 29-bit limbs) over `curve`'s base field, every CU busy with `waves_per_simd` waves per SIMD; measured
 * chip-wide modmul/s (best of three launches).  bench.py reports it as `modmul_ceiling`. */
int h2_selftest_modmul_rate(int curve, int waves_per_simd, int iters, double* modmul_per_s);
/* host-only pieces of the product surface, for the CPU tests (no GPU, no h2_init needed):
 * what = 0: Blake2b-512 of `in` with the transcript's personalisation ("Halo2-Transcript") -> 64 bytes;
 * 1: the Poseidon constants over bn256::Fr (68 x 3 round constants, MDS, inverse MDS; 32-byte canonical LE each);
 * 2 / 3 / 4: circuit 0 / 1 / 2's verifying-key digest for k = in[0] and the commitments in[1..] (64 canonical bytes
 *    x || y per fixed column then per permutation column, zero = identity) -> 32-byte transcript_repr || the Debug string;
 * 5: pairing check e(P1, Q1) e(P2, Q2) == 1 on two pairs of 64 + 128 canonical bytes -> one byte;
 * 6: the quotient program of circuit in[0] as the prover compiles it -> six u32 (instructions, products, column reads,
 *    live-value slots, constants, inserted reductions) followed by the instructions (3 x u32 each: op_dst, a, b);
 * 7: a caller's expression DAG compiled by the same compiler -> what 6 returns, then the program's constant table
 *    (32-byte canonical LE each: the caller's constants merged by value, plus the one the compiler adds).  The DAG:
 *    u32 nodes, u32 constants, then per node four i32 {op, a, b, x} -- op 0: constant x; 1: column a at rotation x;
 *    2 / 3 / 4: add / sub / mul of the EARLIER nodes a and b -- then the constants (32-byte canonical LE, bn256::Fr).
 *    The last node is the root.  H2_EINVAL for a later or unknown node, a rotation outside [-128, 127], a column
 *    index of 2^22 or more, or a root that is a bare constant or column;
 * 8: the host instantiation of the G1 decompression routine (csrc/h2_decompress.hpp): n x 32 bytes in the wire form ->
 *    n x (64 canonical LE bytes x || y, then the status byte of the public decompression entry point in h2hip.h).;
 * 9: the opening plan of circuit in[0] for k = in[1], as keygen builds it (csrc/h2_opening.hpp): which polynomial is
 *    evaluated and opened at which rotation of x, and where a proof's compressed points sit.  Little-endian: five u32
 *    {1 if the circuit opens with SHPLONK, leading commitments, evaluations E, opening points, opening queries Q}; the
 *    byte offsets of the proof's compressed points (u32 each: leading commitments + opening points of them, ascending);
 *    E records of three i32 {kind, index, rotation} in the order the evaluations go onto the transcript; Q records of
 *    four i32 {kind, index, rotation, index of the query's evaluation among the E, -1 for h} in the batching order of
 *    the multi-open.  kind: 0 advice, 1 fixed, 2 sigma, 3 permutation product, 4 random polynomial, 5 h; index: the
 *    column, the permutation column or the product's set; rotation in rows (signed);
 * 10: the host instantiation of the Pasta decompression routine (csrc/h2_decompress.hpp, pasta_decompress): one curve byte
 *    (1 = Pallas, 2 = Vesta; BN254 is H2_EINVAL), then n x 32 bytes in the Pasta wire form -> n x (64 canonical LE bytes
 *    x || y, then the status byte of h2_pasta_points_decompress_device);
 * 11: the host instantiation of the base field's square root (csrc/h2_sqrt.hpp): one curve byte (0, 1 or 2), then n x 32
 *    little-endian field elements (one that is not canonical is handed on as it is, to be refused) -> n x (32 canonical LE
 *    bytes of the root, then the status byte of h2_base_sqrt_device). */
/* commit phases of the C++ prover / keygen that were spread over more than one context (h2_init_devices) so far */
uint64_t h2_selftest_sharded_commits(void);
/* rows per context from which the C++ prover spreads a commit phase over the contexts (default 1024; 0 restores it) */
int h2_selftest_set_shard_min_rows(size_t rows);
/* commit phases (MSM launch sequences with their read-back) the C++ prover and keygen have started since the library was
 * loaded: h2_generate_proofs makes as many for a group of proofs as h2_generate_proof makes for one */
uint64_t h2_selftest_commit_launches(void);
/* proofs that h2_generate_proofs runs in lockstep; a larger batch is cut into groups of this many (0 restores the default) */
int h2_selftest_set_prove_group(size_t proofs);
int h2_selftest_host(int what, const uint8_t* in, size_t in_len, uint8_t* out, size_t cap, size_t* out_len);
/* the 29-bit working-form product (h2_field29.hpp) instantiated on the host, no GPU: field 0 bn254 Fq, 1 bn254 Fr,
 * 2 pasta Fp, 3 pasta Fq; in = four operands a, b, c, d of 9 signed 29-bit-radix limbs; op 0: fe29_mul(a, b),
 * 1: fe29_sqr(a), 2: fe29_mul_sub(a, b, c, d), 3: fe29_mul_up(a, b) -> the 9 limbs of the result */
int h2_selftest_fe29_op(int field, int op, const int32_t in[36], int32_t out[9]);
/* the same four ops through the DEVICE instantiation: n operand sets (36 limbs each, host pointer) -> n x 9 limbs,
 * one kernel launch */
int h2_selftest_fe29_op_device(int field, int op, const int32_t* in, int32_t* out, size_t n);
/* the same four ops through BOTH device forms of the product, Pasta fields only (field 2 or 3): out_cpp = the compiler's
 * form (h2_field29.hpp), out_chain = the single-chain form the accumulate kernel and the NTT pass use
 * (h2_field29_chain.hpp); n x 9 limbs each, one kernel launch.  The two must be equal limb for limb */
int h2_selftest_fe29_chain_device(int field, int op, const int32_t* in, int32_t* out_cpp, int32_t* out_chain, size_t n);
/* the working-form group law (csrc/h2_curve29.hpp) on RAW operands, instantiated on the host, no GPU and no h2_init:
 * in = operand A then operand B, each a stored XYZZ point (x, y, zz, zzz of 9 signed 29-bit-radix limbs, anywhere in the
 * ranges of the stored-point contract at the top of h2_curve29.hpp); for the affine ops B's first 18 limbs are (x, y)
 * and the rest is ignored.  op 0: xyzz29_add(A, B), 1: xyzz29_double(A), 2: xyzz29_add_affine(A, b),
 * 3: xyzz29_double_affine(b), the affine ops on the default product policy -> the result's 36 limbs exactly as
 * xyzz29_store writes them (no conversion, no normalisation added) */
int h2_selftest_xyzz29_op(int curve, int op, const int32_t in[72], int32_t out[36]);
/* the same through the DEVICE instantiation: n operand pairs (72 limbs each, host pointer), one kernel launch, four
 * lanes per pair; out = n x 4 x 36 limbs: EVERY lane of the quad writes its own copy of the result.  op 0..3 as on the
 * host (the one-lane forms run in all four lanes on the same data), 4: xyzz29_add_quad(A, B), 5: xyzz29_double_quad(A)
 * (csrc/h2_curve_quad.hpp), 6 / 7: xyzz29_add_affine / xyzz29_double_affine on the single-chain products as the
 * accumulate kernel instantiates them (Fe29Chain) -- only where that form exists (Pallas, Vesta); H2_EINVAL and
 * nothing written for BN254.  The limbs of 6 / 7 must equal those of 2 / 3 */
int h2_selftest_xyzz29_op_device(int curve, int op, const int32_t* in, int32_t* out, size_t n);
/* the quotient program's kernel (expr_kernel) on a caller's DAG (the format of h2_selftest_host what = 7), launched
 * as the prover launches it: ncols host columns, concatenated, column c of 2^log_len[c] elements (4 x u64, x 2^256
 * canonical) read at row (i + rot * step) & (2^log_len[c] - 1); out = the 2^log_en results (4 x u64 each, canonical);
 * stats = what 6's six counters.  H2_EINVAL (nothing launched) for what what 7 refuses, a column that does not exist,
 * an element that is not canonical, or a program that needs more LDS than one workgroup may hold. */
int h2_selftest_expr_run(const uint8_t* dag, size_t dag_len, const uint64_t* cols, const uint32_t* log_len, uint32_t ncols,
                         uint32_t log_en, uint32_t step, uint64_t* out, uint32_t stats[6]);
/* scratch arenas of the current context: out = {allocations, cross-stream hand-overs (event waits), MSM slots taken
 * over by a further stream, NTT slots taken over} since h2_init */
int h2_selftest_arena_stats(uint64_t out[4]);
/* pairing checks the two verify entry points of the product surface have made since the library was loaded */
uint64_t h2_selftest_pairing_checks(void);
/* Poseidon (h2_poseidon_*; csrc/h2_poseidon.hpp).
 * h2_selftest_poseidon: host only, no GPU and no h2_init -- the kernels' permutation template instantiated on the host,
 *   over `curve`'s scalar field with the constants of (r_f, r_p).  op 0: in = one state of 3 elements -> out = the permuted
 *   state; op 1: in = two elements -> out = their ConstantLength<2> hash (one element).  4 x u64 Montgomery limbs each,
 *   canonical.  H2_EINVAL for what h2_poseidon_constants refuses or another op.
 * h2_selftest_set_poseidon_merkle_tail: tests and tools only -- the widest level h2_poseidon_merkle_device leaves to its
 *   single-workgroup launch: a power of two up to 512; 0 restores the default.  h2_poseidon_merkle_tail() reports the value
 *   in force.
 * h2_selftest_set_poseidon_form: tests and tools only -- the form of the field product in the hash launches of
 *   h2_poseidon_hash_device and h2_poseidon_merkle_device: 1 = the compiler's form at every size, 2 = the single-chain form
 *   (csrc/h2_field29_chain.hpp) at every size where the field has one (Pallas, Vesta), 0 restores the choice by size
 *   (single-chain from 2^16 + 1 lanes on).  The results are the same limb for limb.  H2_EINVAL for another value. */
int h2_selftest_poseidon(int curve, uint32_t r_f, uint32_t r_p, int op, const uint64_t* in, uint64_t* out);
/* Poseidon items from which h2_verify_proofs computes the batch's public inputs with one h2_poseidon_hash_device launch
 * instead of one host permutation per item; a smaller batch hashes on the host as h2_verify_proof does.  0 restores the
 * default; SIZE_MAX keeps every batch on the host. */
int h2_selftest_set_poseidon_verify_min(size_t count);
int h2_selftest_set_poseidon_merkle_tail(uint32_t nodes);
int h2_selftest_set_poseidon_form(int form);
/* tests and tools only -- the form of h2_poseidon_merkle_verify_device's walker and of the level and top launches of
 * h2_poseidon_merkle_update_device: 1 = one lane per hash at every size, 2 = the four lanes of a quad per hash at every
 * size, 0 = by size (the default).  The results are the same bits either way.  H2_EINVAL for another value. */
int h2_selftest_set_poseidon_walk_form(int form);
/* The wide Poseidon family (h2_poseidon_wide_*; csrc/h2_poseidon.hpp), widths 5 and 9.
 * h2_selftest_poseidon_wide_table: host only, no GPU and no h2_init -- the whole table the kernels read, as 4 x u64
 *   Montgomery limbs: h2_poseidon_wide_constants' (r_f + r_p) * width + width^2 elements, then the SPARSE form of the partial
 *   rounds: the width x width pre-matrix (row-major) that the last full round in front of them takes in place of the MDS;
 *   the `width` constants added to the state in front of partial round 0 (element 0 of them is round 0's `a`); per partial
 *   round 2 * width + 1 elements (a, b, m00, vhat[1 .. width - 1], w[1 .. width - 1]) for
 *       z = (s_0 + a)^5 + b;   s_0 <- m00 z + sum_j vhat_j s_j;   s_j <- s_j + w_j z   (j >= 1, the old s_j in the sum);
 *   and the field's one.  *n_elems as h2_poseidon_wide_constants reports it.  H2_EINVAL for a width other than 5 or 9 and
 *   for what h2_poseidon_wide_constants refuses.
 * h2_selftest_poseidon_wide: host only -- the kernels' templates instantiated on the host over that table.  op 0: in = one
 *   state of `width` elements -> out = the permuted state (len ignored); op 1: in = len elements -> out = their
 *   ConstantLength<len> hash.  form 0 = the width's own partial rounds, 1 = dense, 2 = sparse (op 1: the width's own only).
 * h2_selftest_set_poseidon_wide_form: tests and tools only -- the partial rounds of h2_poseidon_wide_permute_device's kernel,
 *   form as above; the results are the same bits.  Every other wide launch runs the width's own form. */
int h2_selftest_poseidon_wide_table(int curve, uint32_t width, uint32_t r_f, uint32_t r_p, uint64_t* out, size_t cap_elems,
                                    size_t* n_elems);
int h2_selftest_poseidon_wide(int curve, uint32_t width, uint32_t r_f, uint32_t r_p, int form, int op, uint32_t len,
                              const uint64_t* in, uint64_t* out);
int h2_selftest_set_poseidon_wide_form(int form);
/* The IPA prover's transcript step (h2_ipa_prove_rounds_device; csrc/h2_ipa_prove.hpp): the host instantiation of what one
 * lane of the step kernel runs, no GPU and no h2_init.  form 0: the inversion by a fixed number of divsteps (the
 * product's), 1: fe_inv's Fermat chain.
 * h2_selftest_field_inv: field as h2_selftest_field_op; a, out: 4 x u64 Montgomery limbs; out = 1 / a, and 0 for a = 0.
 * h2_selftest_ipa_step: the lane's work behind a round on `curve` (H2_PALLAS or H2_VESTA; H2_EINVAL otherwise).  state_in:
 *   the 208 bytes of the midstate; lr: L || R, affine, 16 Montgomery limbs of the base field, (0, 0) the identity; lrf: the
 *   round's blinds l, r and f as it stands (Montgomery limbs of the scalar field) -> wire: the two 32-byte wire forms;
 *   state_out: the midstate behind the squeeze; out = u || 1 / u || f + l / u + r u; *status = 1 if u = 0, else 0.
 * h2_selftest_ipa_fold: the part of that behind the squeeze on a caller's u: in = u || l || r || f ->
 *   out = 1 / u || f + l / u + r u, *status as above (u = 0: out = 0 || f, *status = 1).
 * h2_selftest_ipa_step_scalar: the lane's common_scalar behind the final kernel: s (Montgomery limbs) -> canon, its 32
 *   canonical little-endian bytes as they go to the proof; state_out: the midstate behind 0x02 || canon.
 * h2_selftest_set_ipa_inv_form: tests and tools only -- the inversion the step kernel launches with from now on. */
int h2_selftest_field_inv(int field, int form, const uint64_t a[4], uint64_t out[4]);
int h2_selftest_ipa_step(int curve, int form, const uint8_t state_in[208], const uint64_t lr[16], const uint64_t lrf[12],
                         uint8_t wire[64], uint8_t state_out[208], uint64_t out[12], uint32_t* status);
int h2_selftest_ipa_fold(int curve, int form, const uint64_t in[16], uint64_t out[8], uint32_t* status);
int h2_selftest_ipa_step_scalar(int curve, const uint8_t state_in[208], const uint64_t s[4], uint8_t canon[32],
                                uint8_t state_out[208]);
int h2_selftest_set_ipa_inv_form(int form);

#ifdef __cplusplus
}
#endif
#endif
