/*
 * h2hip.h -- C ABI of the MI355X (gfx950) MSM / NTT backend for halo2.
 *
 * Drop-in boundary for the hot path of 0xWOLAND/halo2-prover: the calls
 * halo2_proofs::plonk::create_proof / keygen_{vk,pk} make into
 *   halo2_proofs::arithmetic::best_multiexp   (via ParamsKZG::commit / commit_lagrange)
 *   halo2_proofs::arithmetic::best_fft        (via EvaluationDomain::{lagrange_to_coeff,
 *                                              coeff_to_extended, extended_to_coeff})
 * when driven by the reference's circuits/ crate:
 *   /root/reference/circuits/src/utils.rs:63-70   (keygen)        -> fixed/sigma commitments
 *   /root/reference/circuits/src/utils.rs:83-91   (SHPLONK prove) -> create_proof
 *   /root/reference/circuits/src/utils.rs:105-120 (GWC prove)     -> create_proof
 *   /root/reference/circuits/src/wasm.rs:57-65,77-122             -> same, behind wasm-bindgen
 * The functions themselves live in the un-vendored dependency halo2_proofs @6b43b6b
 * (circuits/Cargo.toml:16-17, Cargo.lock:836-838); their Rust signatures are restated in
 * SURVEY.md section 8(b).  INTEGRATION.md shows the Rust-side `extern "C"` binding.
 *
 * Conventions (identical to halo2curves' in-memory layout, so a Rust slice can be passed as is):
 *   field element  = 4 x u64 little-endian limbs, Montgomery form (R = 2^256)      32 bytes
 *   affine point   = x || y, identity = (0, 0)                                     64 bytes
 *   Jacobian point = x || y || z, identity has z = 0                               96 bytes
 * All functions return 0 on success or a negative h2_status_t; they never abort or throw
 * across the ABI (the reference panics on length mismatch; here that is H2_EINVAL).
 *
 * Threading and streams.  Every entry point takes one process-wide lock while it validates and ENQUEUES, so calls
 * from several host threads are safe.  Host-pointer entry points run on the library's own stream of each device and
 * return when the result is in host memory.  The *_device entry points enqueue on the caller's `stream` (a
 * hipStream_t; NULL = the library's stream, a blocking stream, i.e. ordered against the legacy null stream that
 * PyTorch uses by default) and return without synchronising.  Different calls may use different streams.  The MSM
 * workspace and the multi-pass NTT's second buffer exist once per stream for up to four streams per device: MSMs (or
 * NTTs) enqueued on different streams run side by side -- two proofs in flight on one GPU, DESIGN.md section 5 -- and a
 * fifth stream takes over the scratch that has been idle longest, behind an event wait.  The division / prefix-scan
 * scratch is one per device: it remembers its last user and makes a call on another stream wait for it.  Results are
 * correct whatever streams are mixed (tests/test_gpu_multi.py).  Scratch is sized by the largest call seen on its
 * stream and kept until h2_shutdown.
 * The caller orders its own producers / consumers of the device buffers it passes, as with any HIP library.
 *
 * Devices.  h2_init(device) binds the process to one GPU (one process per GPU under torch.distributed / RCCL is how
 * the Python host layer scales out).  h2_init_devices(n, ids) gives ONE process several GPUs
 * (the shape a Rust host linking this library wants): bases are replicated on every device at registration,
 * h2_msm_batch / h2_ntt_batch shard their columns column j -> device j mod n, h2_msm splits one long MSM by
 * contiguous point range and adds the n partial sums; results travel as 64/96-byte points through host memory, so
 * no device-to-device collective is needed inside one process.  *_device entry points act on the context of the
 * calling thread's current HIP device.  The product surface uses the contexts too: h2_generate_proof (keygen and
 * create_proof) spreads every commit phase over them by point range -- context g commits rows [n g / G, n (g+1) / G)
 * of every column of the phase against its replica of the table; the other contexts' shares of the columns and the
 * G x m partial sums travel device to device (peer copies) and the sums are added on the prover's device -- and
 * produces the same proof bytes as with one context (tests/test_gpu_multi.py).
 *
 * Trust.  h2_generate_proof / h2_verify_proof keep the SRS tables and keys of the last few params blobs and recognise a
 * blob by a fast fingerprint (eight multiply-xorshift lanes over every byte, finished through Blake2b with the header
 * and the G2 tail): it guards against accidents, NOT against a party who crafts a second blob to collide with a cached
 * one.  Params must come from a source the caller trusts (as the reference's own flow assumes: the UI generates them);
 * a verifier that takes params from an untrusted party calls h2_params_cache_clear() before h2_verify_proof.
 */
#ifndef H2HIP_H
#define H2HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum { H2_BN254 = 0, H2_PALLAS = 1, H2_VESTA = 2 } h2_curve_t;

typedef enum {
  H2_OK = 0,
  H2_EINVAL = -1,   /* bad argument: length / log_n mismatch, null pointer, unknown curve */
  H2_ENOMEM = -2,   /* host or device allocation failed */
  H2_EDEVICE = -3,  /* HIP runtime error (no device, launch failure, ...) */
  H2_EHANDLE = -4,  /* unknown or released bases handle */
  H2_ENOTINIT = -5, /* h2_init has not been called */
  H2_EPROOF = -6    /* the product surface (h2_generate_proof / h2_verify_proof ...): malformed input or proof */
} h2_status_t;

/* ---- lifecycle -------------------------------------------------------------------------- */
/* Bind this process to one GPU (HIP device ordinal).  Idempotent for the same device. */
int h2_init(int device);
/* One process, several GPUs (SURVEY.md section 8(b) `h2_init(n_devices, ids)`): one context, stream and set of
 * arenas per listed device.  Idempotent for the same list.  An id may be listed twice (two contexts on one GPU:
 * how the sharded paths are tested on a one-GPU box). */
int h2_init_devices(int n_devices, const int* device_ids);
/* number of contexts, or H2_ENOTINIT */
int h2_device_count(void);
int h2_shutdown(void);
const char* h2_strerror(int status);
/* Text of the last HIP error seen by this process ("" if none). */
const char* h2_last_device_error(void);
/* ABI version: major * 1000 + minor. */
int h2_version(void);

/* ---- bases (the SRS: ParamsKZG::g / g_lagrange) ------------------------------------------
 * Registers n affine points and keeps them -- plus the table of their 2^(c*w) multiples that
 * lets every Pippenger window share one bucket set -- resident in HBM.  Replaces the `bases`
 * slice argument of best_multiexp for all later calls (ParamsKZG::commit_lagrange passes
 * g_lagrange, ParamsKZG::commit passes g).  `affine` is a host pointer.  Every point must be the
 * identity (0, 0) or lie on the curve with canonical coordinates (checked on the device while the table is built, as
 * the reference's ParamsKZG::read checks with SerdeFormat::RawBytes): otherwise H2_EINVAL. */
int h2_bases_register(h2_curve_t curve, const uint64_t* affine /* n*8 */, size_t n, uint64_t* handle_out);
/* Same, from a device pointer (the points are copied; the caller keeps ownership). */
int h2_bases_register_device(h2_curve_t curve, const void* d_affine, size_t n, uint64_t* handle_out);
int h2_bases_release(uint64_t handle);
/* Number of points registered under the handle, or a negative status. */
int64_t h2_bases_len(uint64_t handle);

/* ---- MSM == best_multiexp(coeffs, bases) -> C::Curve ------------------------------------
 * out_jac receives sum_i scalars[i] * bases[i] as a Jacobian point (any representative of
 * the group element; compare after normalisation).  n may be smaller than the registered
 * length (a prefix of the bases is used), never larger. */
int h2_msm(h2_curve_t curve, uint64_t bases_handle, const uint64_t* scalars /* n*4 */, size_t n,
           uint64_t out_jac[12]);
/* m columns against the same bases (the per-column commitments of one proof phase).
 * out_affine receives m normalised affine points (identity = (0,0)), column order. */
int h2_msm_batch(h2_curve_t curve, uint64_t bases_handle, const uint64_t* const* scalars /* m ptrs */,
                 size_t n, size_t m, uint64_t* out_affine /* m*8 */);
/* Device-resident form: d_scalars holds m columns of n scalars, column stride n*32 bytes;
 * d_out_jac receives m Jacobian points (m*96 bytes, device memory).  Enqueued on `stream`
 * (a hipStream_t, NULL = the library's stream); returns without synchronising. */
int h2_msm_device(h2_curve_t curve, uint64_t bases_handle, const void* d_scalars, size_t n, size_t m,
                  void* d_out_jac, void* stream);
/* m columns, column j against the bases registered under handles[j] (all of the same length and curve; m <= 16):
 * ONE launch sequence for commitments that do not wait for each other although they use different SRS vectors --
 * in create_proof the permutation products (over g_lagrange) and the vanishing argument's random polynomial (over g,
 * drawn from the RNG, not from the transcript).  first_base / n / col_stride as in h2_msm_device_range.  Every MSM call pays ~0.3 ms of sort + small-grid tail whatever m is. */
int h2_msm_device_multi(h2_curve_t curve, const uint64_t* bases_handles /* m */, const void* d_scalars,
                        size_t first_base, size_t n, size_t col_stride, size_t m, void* d_out_jac, void* stream);
/* Make `stream` wait until the bucket-accumulate kernel of the most recently enqueued MSM (on any stream) has
 * finished.  What follows it in an MSM -- the per-bucket fix-up, the bucket weights, the tree sums -- are chains of
 * dependent point operations on about one wave per SIMD: work queued on another stream behind this wait (the
 * Lagrange -> coefficient -> extended transforms of columns whose commitment is being computed) runs beside them
 * instead of beside the chip-filling accumulate kernel.  The first call only switches the marking on (no MSM has
 * recorded its point yet, so nothing is waited for); bench.py's warm-up steps absorb that. */
int h2_stream_wait_msm_tail(void* stream);
/* The same over a contiguous RANGE of the registered bases: result_j = sum_{i<n} scalars_j[i] * bases[first_base + i],
 * columns col_stride elements apart (col_stride >= n).  This is one rank's share of an MSM split by point range over
 * several GPUs (BASELINE config 4): every rank passes its slice of every column, the
 * partial sums are all-gathered (96 B each) and added with h2_points_sum_device. */
int h2_msm_device_range(h2_curve_t curve, uint64_t bases_handle, const void* d_scalars, size_t first_base, size_t n,
                        size_t col_stride, size_t m, void* d_out_jac, void* stream);
/* d_out_jac[j] = sum_{g < groups} d_in_jac[g * count + j] for j < count (Jacobian points, device memory): adds the
 * all-gathered partial sums of a range-split MSM.  d_out_jac must not alias d_in_jac. */
int h2_points_sum_device(h2_curve_t curve, const void* d_in_jac, size_t groups, size_t count, void* d_out_jac,
                         void* stream);

/* ---- MSM over points passed WITH the call: best_multiexp(coeffs, bases) for bases that are NOT registered ----------
 * out_j = sum_{i<n} scalars_j[i] * points[i].  points: n affine points (64 bytes, API form, identity = (0,0));
 * m scalar columns col_stride elements apart (col_stride >= n); d_out_jac: m Jacobian points (identity: z = 0; any
 * representative of the group element, compare after normalisation).  No table is built or kept: a bucket MSM with a
 * bucket set per window, the window results combined by doublings at the end.  This is the call for a slice used once -- a
 * sub-slice, a one-off vector, a verifier's terms, an SRS read for a single proof; bases that many MSMs share belong in
 * h2_bases_register, whose table makes each of those MSMs cheaper.
 *
 * Streams and scratch.  h2_msm_points_device is asynchronous on `stream` under h2_msm_device's rules: it uses the
 * stream's MSM workspace slot, the points in their working form live in that scratch too, and nothing outlives the call
 * (no handle, no table, no entry in any map).  h2_msm_points takes host pointers, runs on the library's stream of the
 * current context and returns with the result in host memory.
 * Contexts.  With several contexts (h2_init_devices) both forms act on ONE context -- that of the calling thread's
 * current HIP device -- and do not shard; a caller splits by point range and adds with h2_points_sum_device, as for
 * h2_msm_device_range.
 * Point validity.  The points are NOT checked to be on the curve (best_multiexp does not check either).  Every index
 * the kernels form depends on the scalars and on n only, so a bad point gives a wrong sum and never an out-of-range
 * access.  h2_bases_register stays the checked route.
 * Sizes.  Every n from 0 up to 2^26 (h2_msm_points_plan_t.max_n: a column's sorted entries are indexed with 31 bits);
 * below h2_msm_points_plan_t.crossover terms the call takes a double-and-add route (one quad of lanes per term),
 * from there on buckets.  m is not limited: wide batches run in groups of columns on the same stream.
 * Returns.  H2_ENOTINIT before h2_init.  H2_EINVAL, checked on the host before anything is enqueued: a null pointer
 * with n > 0 && m > 0 (d_out_jac: with m > 0), col_stride < n, an unknown curve, a device pointer that is not 16-byte
 * aligned, n > 2^26.  m == 0: H2_OK, nothing enqueued.  n == 0: H2_OK, m identities are written.  H2_EDEVICE with the
 * violated condition in h2_last_device_error if the host-side bounds proof of the launch sequence fails (nothing is
 * enqueued then). */
int h2_msm_points_device(h2_curve_t curve, const void* d_points, const void* d_scalars, size_t n, size_t col_stride,
                         size_t m, void* d_out_jac, void* stream);
int h2_msm_points(h2_curve_t curve, const uint64_t* points /* n*8 */, const uint64_t* scalars /* n*4 */, size_t n,
                  uint64_t out_jac[12]);
/* Geometry the calls above would use for n terms.  Host only: no GPU, no h2_init needed.  H2_EINVAL: unknown curve, null
 * `out`, n > 2^26. */
typedef struct {
  uint32_t window_bits;   /* widest window c */
  uint32_t windows;       /* W: windows of a scalar = bucket sets per column */
  uint32_t buckets;       /* per window: 2^(c-1) */
  uint32_t route;         /* 0 = the double-and-add route for short inputs (n < crossover), 1 = buckets */
  uint32_t scalar_bits;   /* the windows cover scalar_bits + 1 bits */
  uint32_t lds_bytes;     /* W * buckets * 4: the sort front's histogram per workgroup ... */
  uint32_t lds_limit;     /* ... and what it may use */
  uint32_t reserved;
  uint64_t crossover;     /* terms from which the bucket route is taken */
  uint64_t max_n;         /* the largest n a call takes */
  uint8_t width[48];      /* bits of window w, w < windows */
  uint8_t offset[48];     /* first bit of window w */
} h2_msm_points_plan_t;
int h2_msm_points_plan(h2_curve_t curve, size_t n, h2_msm_points_plan_t* out);

/* n compressed G1 points (32 bytes each: x little-endian, bit 6 of the last byte = parity of y, bit 7 = identity flag --
 * the wire form of Blake2bRead / Blake2bWrite) -> n affine points in the API form (64 bytes,
 * Montgomery limbs) and n status bytes: 0 = a point on the curve, 1 = x not canonical (>= q), 2 = the identity
 * (flag set, or x = 0 with parity 0), 3 = x^3 + 3 is not a square.  For status != 0 the 64 output bytes are zero.
 * One lane per point takes y = (x^3 + 3)^((q + 1) / 4), which needs q = 3 mod 4: H2_BN254 only, other curves H2_EINVAL.
 * Device pointers; d_compressed and d_out_affine 16-byte aligned (H2_EINVAL otherwise); asynchronous on `stream`. */
int h2_points_decompress_device(h2_curve_t curve, const void* d_compressed, size_t n, void* d_out_affine,
                                void* d_status, void* stream);

/* square roots in the BASE field of `curve` (all three curves): n elements (4 x u64 Montgomery limbs) -> n roots and n status
 * bytes: 0 = root written (of the two, the one whose canonical integer is even; 0 for 0), 1 = input not canonical,
 * 3 = not a square.  For status != 0 the 32 output bytes are zero.  d_out may equal d_in exactly.  One lane per element, the
 * same instructions for every element (csrc/h2_sqrt.hpp: BN254 by one power, the Pasta fields -- q = 1 mod 2^32 -- by a power
 * and a discrete logarithm in the 2^32-th roots of unity, four bits at a time by table).
 * Device pointers; d_in and d_out 16-byte aligned; n <= 2^30; an output that partly overlaps an input is H2_EINVAL, as is
 * every other bad argument, before anything is enqueued; n = 0 enqueues nothing; asynchronous on `stream`. */
int h2_base_sqrt_device(h2_curve_t curve, const void* d_in, size_t n, void* d_out, void* d_status, void* stream);
/* h2_points_decompress_device for the Pasta wire form (transcript.py: x little-endian, bit 255 the parity of y, 32 zero
 * bytes the identity; no identity flag): H2_PALLAS and H2_VESTA only, H2_BN254 is H2_EINVAL.  Same outputs and status
 * codes 0 / 1 / 2 / 3; decision and coordinates are transcript.decompress's for EVERY 32-byte input.  Same pointer rules;
 * no output may overlap the input. */
int h2_pasta_points_decompress_device(h2_curve_t curve, const void* d_compressed, size_t n, void* d_out_affine,
                                      void* d_status, void* stream);

/* ---- NTT == best_fft(a, omega, log_n) ---------------------------------------------------
 * In place, natural order in and out, A[i] = sum_j a[j] * omega^(i*j), unscaled, over the
 * SCALAR field of `curve` (bn256::Fr for H2_BN254).  a must hold exactly 1 << log_n elements. */
int h2_ntt(h2_curve_t curve, uint64_t* a /* n*4, in place */, const uint64_t omega[4], uint32_t log_n);
int h2_ntt_batch(h2_curve_t curve, uint64_t* const* cols /* m ptrs */, size_t m, const uint64_t omega[4],
                 uint32_t log_n);
/* Device-resident form: m columns, column stride (1 << log_n) * 32 bytes, in place. */
int h2_ntt_device(h2_curve_t curve, void* d_a, size_t m, const uint64_t omega[4], uint32_t log_n,
                  void* stream);

/* ---- EvaluationDomain pieces (halo2_proofs/src/poly/domain.rs) ----
 * Device-resident columns (m columns, stride n*32 bytes) over the SCALAR field of `curve`; asynchronous on
 * `stream` (NULL = the library's stream).  With these a column stays in HBM from its Lagrange form through
 * lagrange_to_coeff / coeff_to_extended / divide_by_vanishing_poly / extended_to_coeff to its commitment. */
/* best_fft followed by a[i] *= scale, fused into the last pass: EvaluationDomain::ifft(a, omega_inv, k, n^-1) */
int h2_ntt_scaled_device(h2_curve_t curve, void* d_a, size_t m, const uint64_t omega[4], uint32_t log_n,
                         const uint64_t scale[4], void* stream);
/* EvaluationDomain::coeff_to_extended.  m columns of n = 2^log_n coefficients, column stride col_stride elements
 * (col_stride >= n), over the SCALAR field of `curve`  ->  m columns of 2^ext_log_n values, column stride 2^ext_log_n:
 *   out[c][i] = sum_{j < n} in[c][j] * z[j mod 3] * ext_omega^(i*j),   z = {1, zeta, zeta^2}
 * i.e. halo2's distribute_powers_zeta (for zeta^3 = 1 this is zeta^j) then best_fft on the zero-extended column.
 * Out of place: the source is read only, d_out must not overlap it.  Canonical output, natural order.
 * Asynchronous on `stream`.
 * The zero-extended column is never written or read: the first NTT pass loads the n coefficients from the source,
 * multiplies by zeta^j on the way in and treats the rest of its tile as zero -- no pad, copy or coset launch.  Stream
 * and scratch rules are h2_ntt_device's (the same twiddle tables, keyed by (ext_omega, ext_log_n); a multi-pass plan
 * uses the stream's second buffer of m * 2^ext_log_n elements); no other device memory is allocated.
 * H2_EINVAL -- checked on the host before anything is enqueued -- for: a null pointer with m > 0, ext_log_n < log_n,
 * ext_log_n > 30 (h2_ntt_device's limit), col_stride < n, m > 65535, byte ranges of source and destination that
 * overlap.  m = 0 is H2_OK and enqueues nothing; ext_log_n == log_n is legal (a coset shift plus an out-of-place NTT).
 * h2_version() did not change for this entry point: a host detects it by its symbol, as with h2_generate_proofs. */
int h2_coeff_to_extended_device(h2_curve_t curve, const void* d_coeff, size_t col_stride, uint32_t log_n, size_t m,
                                const uint64_t zeta[4], const uint64_t ext_omega[4], uint32_t ext_log_n,
                                void* d_out, void* stream);
/* EvaluationDomain::extended_to_coeff -- and divide_by_vanishing_poly before it when d_t is given -- in ONE call.
 * m columns of 2^ext_log_n values over the SCALAR field of `curve`, column stride 2^ext_log_n  ->  m columns of out_len
 * coefficients, column stride out_stride elements:
 *   out[c][j] = zi[j mod 3] * scale * sum_{i < 2^ext_log_n} ext[c][i] * t[i mod t_period] * ext_omega_inv^(i*j)
 *               for j < out_len,   zi = {1, zeta_inv, zeta_inv^2}
 * d_t: a device table of t_period canonical Montgomery elements (h2_poly_mul_periodic_device's meaning), or NULL: no
 * factor, t_period ignored.  With scale = 1 / 2^ext_log_n, zeta_inv = g_coset^-1 and out_len = n (j - 1) this is the
 * ifft on the extended domain, the coset un-shift and the truncation.
 * Out of place: the source is read only, d_out must not overlap it.  Canonical output, natural order.  Rows
 * [out_len, out_stride) of every destination column are not touched.  Asynchronous on `stream`.
 * No full-length coefficient column is written, read back or copied: the t factor rides on the first NTT pass's load;
 * the last pass drops an output at or beyond out_len before any arithmetic and multiplies the others by zeta_inv^j
 * (folded into the scale's product where the last pass has one) on their way out.  Stream, scratch and table rules
 * are h2_ntt_scaled_device's: the same twiddle table for the same (ext_omega_inv, ext_log_n, scale), a multi-pass plan
 * uses the stream's second buffer of m * 2^ext_log_n elements; nothing else is allocated, nothing else is cached.
 * H2_EINVAL -- checked on the host before anything is enqueued -- for: a null d_ext, d_out, ext_omega_inv, scale or
 * zeta_inv with m > 0 and out_len > 0; ext_log_n > 30; out_len > 2^ext_log_n; out_stride < out_len (or above 2^40);
 * m > 65535; with d_t, a t_period that is zero, not a power of two or above 2^ext_log_n; a device pointer that is not
 * 16-byte aligned; byte ranges of source and destination that overlap.  m = 0 or out_len = 0 is H2_OK and enqueues
 * nothing; ext_log_n = 0 is legal (out[c][0] = ext[c][0] * t[0] * scale).
 * h2_version() did not change for this entry point: a host detects it by its symbol. */
int h2_extended_to_coeff_device(h2_curve_t curve, const void* d_ext, uint32_t ext_log_n, size_t m,
                                const uint64_t ext_omega_inv[4], const uint64_t scale[4], const uint64_t zeta_inv[4],
                                const void* d_t, size_t t_period,
                                void* d_out, size_t out_len, size_t out_stride, void* stream);
/* The elementwise calls below work in place on canonical Montgomery elements of the SCALAR field of `curve`, asynchronously
 * on `stream`.  Where a call takes n and m, d_a holds m columns of n elements, column stride n.  n * m = 0 (n = 0 where
 * there is no m) is H2_OK and enqueues nothing.  A null d_a, constant, table or d_b, a curve id out of range, a pointwise
 * op outside 0..2 and a period that is zero or no power of two are H2_EINVAL, checked on the host before anything is
 * enqueued and BEFORE the length is looked at: n * m = 0 with one of these is H2_EINVAL, not H2_OK
 * (tests/test_gpu_poly_elementwise.py pins all of this). */
/* a[i] *= c for every i < n * m: the columns are one flat run, m only multiplies the length */
int h2_poly_scale_device(h2_curve_t curve, void* d_a, size_t n, size_t m, const uint64_t c[4], void* stream);
/* a[col][i] *= g^i for i < n, the exponent restarting at 0 in every column: distribute_powers_zeta / the coset shift
 * before an extended-domain NTT (and its inverse) */
int h2_poly_coset_device(h2_curve_t curve, void* d_a, size_t n, size_t m, const uint64_t g[4], void* stream);
/* a[i] *= t[i mod period], period a power of two (else H2_EINVAL): divide_by_vanishing_poly with t = t_evaluations.
 * The index i runs over the FLATTENED n * m elements: column c starts at t[(c * n) mod period], which is t[0] -- the
 * per-column meaning a[col][i] *= t[i mod period] -- exactly when the period divides n.  A period above n * m is legal
 * (no wrap); d_t holds `period` elements and is only read. */
int h2_poly_mul_periodic_device(h2_curve_t curve, void* d_a, size_t n, size_t m, const void* d_t, size_t period,
                                void* stream);
/* a[i] = 1 / a[i] over n elements; a zero element is left as zero, whatever its neighbours hold: the permutation
 * argument's denominators.  There is no m: several columns are one call with n the total. */
int h2_poly_inverse_device(h2_curve_t curve, void* d_a, size_t n, void* stream);
/* a[i] = a[i] op b[i] over n elements; op 0 = add, 1 = sub, 2 = mul, any other op is H2_EINVAL.  d_b == d_a is legal
 * (2a, 0, a^2); d_b is only read. */
int h2_poly_pointwise_device(h2_curve_t curve, int op, void* d_a, const void* d_b, size_t n, void* stream);
/* q = (a - a(z)) / (X - z) over n coefficients, q[n-1] = 0: halo2_proofs src/arithmetic.rs `kate_division(a, z)`
 * (the witness polynomials of the GWC / SHPLONK openings).  d_q must not alias d_a. */
int h2_poly_divide_linear_device(h2_curve_t curve, const void* d_a, size_t n, const uint64_t z[4], void* d_q,
                                 void* stream);
/* out[i] = prod_{j < i} a[j], out[0] = 1 (n elements; d_out may alias d_a): the running product of the permutation
 * argument, z[i+1] = z[i] * ratio[i] (halo2_proofs src/plonk/permutation/prover.rs `Argument::commit`; SURVEY.md
 * App. A.4) -- the caller multiplies by last_z and writes the blinding rows. */
int h2_poly_prefix_product_device(h2_curve_t curve, const void* d_a, size_t n, void* d_out, void* stream);
/* arithmetic.rs eval_polynomial on resident columns: out[t] = sum_{i<n} d_polys[t][i] * points[t]^i for t < q.
 * d_polys: HOST array of q device pointers (n coefficients each, API form, 16-byte aligned; pointers may repeat);
 * points: HOST array of q * 4 limbs; both are read before the call returns.  d_out: q * 32 bytes of device memory,
 * must not overlap any polynomial.  Asynchronous on `stream` under h2_ntt_device's rules.
 * Results are canonical Montgomery limbs, the same bits whatever q and however the jobs are grouped.  0^0 = 1: a zero
 * point returns coefficient 0; n = 0 writes q zeros; q = 0 is H2_OK and enqueues nothing.
 * Three launches per group of jobs (the powers x^16 .. x^T of every point once; one workgroup per T = h2_poly_eval_tile()
 * coefficients: a run of 16 per thread by Horner, the threads' values folded pairwise in LDS; one thread per job folds
 * the tile values by Horner in x^T), job in grid.y.  A group is at most 65535 jobs and at most what keeps its scratch
 * -- (ceil(n / T) * 32 + 324) bytes per job -- under 64 MiB (always at least one job); a larger q runs group after
 * group on `stream`.  That scratch and the job table (40 bytes per job) live in the context's scan arena for the
 * length of the call; nothing is cached.  With several contexts (h2_init_devices) the call acts on the context of the
 * calling thread's current HIP device, as h2_msm_points_device does.
 * H2_EINVAL -- checked on the host before anything is enqueued -- for: an unknown curve, n > 2^30, and with q > 0 a
 * null d_polys, points or d_out, or (n > 0) a d_polys[t] that is null or not 16-byte aligned.
 * h2_version() did not change for these entry points: a host detects them by their symbols. */
int h2_poly_eval_device(h2_curve_t curve, const void* const* d_polys, size_t n, const uint64_t* points, size_t q,
                        void* d_out, void* stream);
/* one host polynomial at one point, synchronous: the drop-in for eval_polynomial(poly, point) */
int h2_poly_eval(h2_curve_t curve, const uint64_t* coeffs /* n*4 */, size_t n, const uint64_t point[4], uint64_t out[4]);
/* coefficients one workgroup covers (T above).  Host only, no h2_init needed: tests size their shapes by it. */
int h2_poly_eval_tile(void);
/* ---- linear combinations of resident columns, with linear factors divided out -----------------------------------
 * The column work of the multiopen argument (GWC's witness polynomials, SHPLONK's h(X) and final quotient) and the join
 * of the quotient pieces h(X) = sum x^(n i) h_i(X), over the scalar field of `curve` (all three curves).  Columns hold n
 * elements in the API form: 4 x u64 Montgomery limbs, canonical in and out.  Per job:
 *     s[i]  = sum_t coeff_t * d_poly_t[i]             i < n, over terms[first_term .. first_term + n_terms); no terms: zeros
 *     s[i] -= low[4 * (first_low + i) ..]             i < n_low: the low coefficients of a remainder
 *     for z in points[4 * (first_point + r) ..], r = 0 .. n_points - 1:   s = kate_division(s, z)
 *                                                     q[i-1] = s[i] + z q[i] from the top, q[n-1] = 0, the remainder
 *                                                     dropped: h2_poly_divide_linear_device's definition
 *     d_out[0 .. n) = s
 * jobs, terms, low and points are HOST arrays, all read before the call returns; d_poly and d_out are device pointers,
 * 16-byte aligned.  Pointers may repeat, within a job and across jobs.  With n_points = 0 a job's d_out may be one of its
 * own term columns (the sum is elementwise); with n_points > 0 it must not overlap any source column.  Two jobs' outputs
 * must not overlap, and a job's output may not be another job's source in the same call.  Nothing beyond d_out[n - 1] is
 * written.  Point 0 is allowed (a shift), a point may repeat.  Results are canonical limbs, the same bits however many
 * jobs share a call and however they are grouped.  Asynchronous on `stream` under h2_ntt_device's rules: no host
 * synchronisation, no device-to-host copy.
 * One launch sums every job of a group (job in grid.y, jobs and terms read from one table in HBM, the `low` subtraction on
 * the same pass); round r of the divisions then runs for every job with n_points > r, eight side by side per launch
 * sequence of three, alternating between an intermediate column and d_out so that the last round lands in d_out.  A
 * group is at most 65535 consecutive jobs and at most as many dividing jobs as keep their intermediate columns (n * 32
 * bytes each) under 256 MiB (always at least one); a wider call runs group after group on `stream`.  The tables (32 bytes
 * per job, 40 per term, 32 per low coefficient), those columns and 8 * 256 KiB of scan values live in the context's scan
 * arena for the length of the call; nothing is cached.  With several contexts (h2_init_devices) the call acts on the
 * context of the calling thread's current HIP device, as h2_poly_eval_device does.
 * n_jobs = 0 or n = 0: H2_OK, nothing enqueued.  H2_EINVAL -- checked on the host before anything is enqueued -- for: an
 * unknown curve; n > 2^30; a job whose ranges run past n_terms, n_low or n_points; a job with n_low > n or n_points >
 * h2_poly_lincomb_max_rounds(); a null or misaligned d_out or d_poly; a null host array that a job refers to; the
 * overlaps ruled out above.  H2_ENOTINIT before h2_init.
 * h2_version() did not change for these entry points, it stays 1002: a host detects them by their symbols. */
typedef struct {
  const void* d_poly;
  uint64_t coeff[4];
} h2_lincomb_term_t; /* 40 bytes */
typedef struct {
  void* d_out;
  uint32_t first_term, n_terms;   /* terms[first_term .. + n_terms) */
  uint32_t first_low, n_low;      /* low[4 * first_low .. + 4 * n_low) */
  uint32_t first_point, n_points; /* points[4 * first_point .. + 4 * n_points), divided out in this order */
} h2_lincomb_job_t; /* 32 bytes */
int h2_poly_lincomb_device(h2_curve_t curve, const h2_lincomb_job_t* jobs, size_t n_jobs, const h2_lincomb_term_t* terms,
                           size_t n_terms, const uint64_t* low, size_t n_low, const uint64_t* points, size_t n_points,
                           size_t n, void* stream);
/* the largest n_points of a job.  Host only, no h2_init needed. */
int h2_poly_lincomb_max_rounds(void);
/* ---- the inner product argument on a registered SRS table --------------------------------------------------------
 * The k rounds of halo2's IPA opening (poly/ipa/commitment/prover.rs create_proof) over the scalar field of `curve` (all
 * three curves), n = 2^k.  The generators are never folded: the folded generators are fixed combinations of the original
 * ones, G^(j)[i] = sum_{h < 2^j} s^(j)[h] G[h 2^(k-j) + i], so L_j and R_j are MSMs over the ORIGINAL table with expanded
 * scalars.  `bases` holds exactly n + 2 points registered ONCE as  G[0 .. n) || U || W;  a round is one two-column MSM of
 * n + 2 terms on it (slot n: z times the round's inner product, slot n + 1: the blind) and O(n) field products.
 * These single calls ARE the lockstep calls below with m = 1 (one code path, the same checks): a state begun by one
 * spelling can be continued by the other.
 *   h2_ipa_state_bytes      size of the caller-owned, 16-byte aligned device buffer one opening works in:
 *                           h2_ipa_batch_state_bytes(k, 1), which describes its contents.  Host only, no h2_init needed.
 *                           H2_EINVAL for k = 0, k > H2_IPA_MAX_K or a null out.
 *   h2_ipa_begin_device     a = the n coefficients d_p (only read), b[i] = x3^i, s = [1].  Whatever an earlier opening
 *                           left in d_state does not matter.
 *   h2_ipa_round_device     round j, 0 <= j < k, half = 2^(k-j-1).  For j > 0 it first folds by the PREVIOUS challenge:
 *                           a[i] += a[i + 2 half] u_prev_inv, b[i] += b[i + 2 half] u_prev, s doubles (s[2h] = s[h],
 *                           s[2h+1] = s[h] u_prev); u_prev and u_prev_inv are both null for j = 0 and both required
 *                           otherwise.  Then  L_j = <a[half..], G'[..half]> + [z <a[half..], b[..half]>] U + [l_blind] W,
 *                           R_j = <a[..half], G'[half..]> + [z <a[..half], b[half..]>] U + [r_blind] W  with G' the folded
 *                           generators.  d_out_affine: 128 bytes, L_j || R_j, affine Montgomery limbs, identity = (0, 0).
 *   h2_ipa_final_device     the last fold, by u_(k-1): d_out = c = a[0], then b[0] (64 bytes); d_s_out (optional, n
 *                           elements) = the finished s = compute_s(u, 1), s[i] = prod over the set bits t of i of u_(k-1-t).
 *   h2_ipa_challenge_products_device   compute_s(u, init) for a verifier: d_out[i] = init prod_{bit t of i} u_(k-1-t);
 *                           u: k * 4 limbs on the HOST, read before the call returns.  <s, G> is then one h2_msm_device.
 * Scalars (x3, z, blinds, challenges) are 4 x u64 Montgomery limbs on the host, canonical, read before the call returns;
 * every output is canonical.  The calls of ONE opening are issued in order -- begin, round 0 .. k - 1, final -- on ONE
 * stream; two openings may run side by side on their own states and streams.  The MSM goes through h2_msm_device's launch
 * path (the stream's workspace slot, the host-side bounds proof, H2_EDEVICE with the violated condition); nothing else is
 * allocated.  Asynchronous on `stream` under h2_ntt_device's rules: no host synchronisation, no device-to-host copy.
 * H2_EINVAL -- checked on the host before anything is enqueued -- for: an unknown curve; k = 0 or k > H2_IPA_MAX_K (bounded
 * by what a registered table of 2^k + 2 bases takes); j >= k; a null or not 16-byte aligned device pointer; a null scalar;
 * a missing or superfluous u_prev / u_prev_inv; a handle of another curve or one that does not hold exactly 2^k + 2 bases
 * (H2_EHANDLE for a handle that is not registered at all).  H2_ENOTINIT before h2_init.
 * h2_version() did not change for these entry points, it stays 1002: a host detects them by their symbols. */
#define H2_IPA_MAX_K 20
int h2_ipa_state_bytes(uint32_t k, size_t* out);
int h2_ipa_begin_device(h2_curve_t curve, uint32_t k, const void* d_p, const uint64_t x3[4], void* d_state, void* stream);
int h2_ipa_round_device(h2_curve_t curve, uint64_t bases, uint32_t k, uint32_t j, void* d_state, const uint64_t* u_prev,
                        const uint64_t* u_prev_inv, const uint64_t z[4], const uint64_t l_blind[4], const uint64_t r_blind[4],
                        void* d_out_affine, void* stream);
int h2_ipa_final_device(h2_curve_t curve, uint32_t k, void* d_state, const uint64_t u_last[4], const uint64_t u_last_inv[4],
                        void* d_out, void* d_s_out, void* stream);
int h2_ipa_challenge_products_device(h2_curve_t curve, const uint64_t* u, uint32_t k, const uint64_t init[4], void* d_out,
                                     void* stream);
/* m openings in lockstep: the calls above for m openings in one state (the calls above are these at m = 1; an opening
 * begun with h2_ipa_begin_device may go on through h2_ipa_round_batch_device with m = 1 and the other way round).
 * ALL m OPENINGS SHARE k, THE CURVE AND THE TABLE `bases`;
 * each has its own polynomial, x3, z, challenges and blinds.  One launch of every kernel serves the m openings and a round is
 * ONE MSM of 2 m columns of n + 2 terms on the registered table (wide batches go through h2_msm_device's column groups), so
 * the launches of a round do not grow with m.  Opening i's outputs are bit for bit what the single-opening calls give.
 *   h2_ipa_batch_state_bytes    size of the caller-owned, 16-byte aligned device buffer m openings work in: per opening a
 *                               and b (two generations each), s and the partial sums; then one block of 2 m columns of
 *                               n + 2; then a table of 5 m scalars every call of m >= 2 fills from its host arguments (at
 *                               m = 1 the scalars travel in the kernels' arguments and the table is neither written nor
 *                               read).  Host only, no h2_init needed.  H2_EINVAL for k = 0, k > H2_IPA_MAX_K, m = 0,
 *                               m > H2_IPA_MAX_BATCH, a null out.
 *   h2_ipa_begin_batch_device   d_p: a HOST array of m device pointers, opening i's n coefficients (only read); x3: m * 4
 *                               limbs.  Whatever an earlier use -- of any m -- left in d_state does not matter.
 *   h2_ipa_round_batch_device   round j of every opening; u_prev, u_prev_inv (both null at j = 0, both required otherwise),
 *                               z, l_blind, r_blind: m * 4 limbs each, entry i for opening i.  d_out_affine: m * 128 bytes,
 *                               L_j || R_j of opening 0, then of opening 1, ...
 *   h2_ipa_final_batch_device   the last fold; u_last, u_last_inv: m * 4 limbs.  d_out: m * 64 bytes, c_i || b_i[0].  The
 *                               finished table s comes from h2_ipa_final_device only.
 * The contract is the single calls': host scalars are canonical Montgomery limbs, read before the call returns (for m >= 2
 * one copy of the scalar table into d_state is enqueued in front of the kernels); the calls of one batch are issued in order on ONE
 * stream; asynchronous on `stream`, no host synchronisation, no device-to-host copy, nothing allocated; the MSM goes through
 * h2_msm_device's launch path with its bounds proof, and what that path refuses with H2_EINVAL (a column too long for the
 * sort's 32-bit indices) is found from the same plans BEFORE the round's table copy and kernels.  H2_EINVAL, before
 * anything is enqueued, for: m = 0 or m >
 * H2_IPA_MAX_BATCH; k = 0 or k > H2_IPA_MAX_K; j >= k; an unknown curve; a null or not 16-byte aligned device pointer, any
 * of the m entries of d_p included; a null scalar array; a missing or superfluous u_prev / u_prev_inv; a handle of another
 * curve or one that does not hold exactly 2^k + 2 bases (H2_EHANDLE for a handle that is not registered at all).
 * h2_version() stays 1002: a host detects these entry points by their symbols. */
#define H2_IPA_MAX_BATCH 64
int h2_ipa_batch_state_bytes(uint32_t k, size_t m, size_t* out);
int h2_ipa_begin_batch_device(h2_curve_t curve, uint32_t k, size_t m, const void* const* d_p, const uint64_t* x3, void* d_state,
                              void* stream);
int h2_ipa_round_batch_device(h2_curve_t curve, uint64_t bases, uint32_t k, uint32_t j, size_t m, void* d_state,
                              const uint64_t* u_prev, const uint64_t* u_prev_inv, const uint64_t* z, const uint64_t* l_blind,
                              const uint64_t* r_blind, void* d_out_affine, void* stream);
int h2_ipa_final_batch_device(h2_curve_t curve, uint32_t k, size_t m, void* d_state, const uint64_t* u_last,
                              const uint64_t* u_last_inv, void* d_out, void* stream);
/* d_out[i] = sum_{p < count} init_p * prod over the set bits t of i of u_p[k-1-t],  i < 2^k: the sum of `count`
 * compute_s(u_p, init_p) vectors, none of them materialised.  u: count * k * 4 limbs, init: count * 4 limbs, HOST, canonical
 * Montgomery, read before the call returns.  Canonical output, the same bits however the proofs are grouped (one launch per
 * 65535 proofs, the later ones adding into d_out).  1 <= k <= H2_IPA_MAX_K; d_out 16-byte aligned; a null u or init with
 * count > 0 is H2_EINVAL; count = 0 writes 2^k zeros. */
int h2_ipa_challenge_products_sum_device(h2_curve_t curve, const uint64_t* u, const uint64_t* init, uint32_t k, size_t count,
                                         void* d_out, void* stream);
/* ---- Poseidon over resident columns: permutation, ConstantLength hash, Merkle tree ---------------------------------
 * The Poseidon primitive of circuits/src/poseidon/primitives*: width 3, rate 2, S-box x^5, r_f full and r_p partial
 * rounds, over the scalar field of `curve` (all three curves), constants from the reference's Grain / Cauchy-MDS
 * generation.  (8, 56) on H2_PALLAS or H2_VESTA is the reference's P128Pow5T3 (the zcash test vectors; Pallas's scalar field
 * is their Fq, Vesta's their Fp); (8, 60) on H2_BN254 is poseidon_circuit.rs's spec, the hash the Poseidon circuit proves.
 * Elements are 4 x u64 Montgomery limbs, canonical (below p) on the way in and on the way out.
 *   h2_poseidon_constants       host only, no device and no h2_init needed: (r_f + r_p) * 3 round constants, then the 3 x 3
 *                               MDS row-major.  *n_elems = the elements that takes, also when cap_elems is too small.
 *   h2_poseidon_permute_device  n states of 3 elements (96 bytes each) -> n states; d_out may be d_in exactly, otherwise
 *                               the two must not overlap.
 *   h2_poseidon_hash_device     ConstantLength<len>: n messages of len elements, msg_stride elements apart, -> n elements.
 *                               The state starts as (0, 0, len 2^64), the message is absorbed two words at a time,
 *                               zero-padded to even length, one permutation per absorb, the output is word 0.
 *   h2_poseidon_merkle_device   2^depth leaves -> the 2^depth - 1 inner nodes, level by level from the leaves' parents up,
 *                               the root last; a node is ConstantLength<2> of its two children.  Levels of more than
 *                               h2_poseidon_merkle_tail() nodes take one launch each, all the levels above them one
 *                               launch of a single workgroup.
 * The device calls are asynchronous on `stream` under h2_ntt_device's rules: no host synchronisation, no device-to-host
 * copy -- except that the FIRST use of a (curve, r_f, r_p) on a context builds its table of constants and waits for
 * that upload; a context keeps the tables of the eight instances used last.  They act on the context of the calling
 * thread's current HIP device.  H2_EINVAL -- checked on the host before anything is enqueued -- for: an unknown curve; r_f
 * odd or 0, or r_f + r_p > H2_POSEIDON_MAX_ROUNDS; a null or not 16-byte aligned device pointer; len = 0 or len > 65535;
 * msg_stride < len or msg_stride > 2^32; n > 2^40; depth = 0 or depth > 30; an output that overlaps an input (other than
 * d_out == d_in of the permutation).  n = 0 is H2_OK and enqueues nothing.  H2_ENOTINIT before h2_init.  h2_version() is unchanged: a host
 * detects these entry points by their symbols. */
#define H2_POSEIDON_MAX_ROUNDS 128      /* r_f + r_p; r_f even and >= 2; r_p >= 0 */
int h2_poseidon_constants(h2_curve_t curve, uint32_t r_f, uint32_t r_p, uint64_t* out, size_t cap_elems, size_t* n_elems);
int h2_poseidon_permute_device(h2_curve_t curve, uint32_t r_f, uint32_t r_p, const void* d_in, void* d_out, size_t n, void* stream);
int h2_poseidon_hash_device(h2_curve_t curve, uint32_t r_f, uint32_t r_p, const void* d_msgs, size_t len, size_t msg_stride,
                            size_t n, void* d_out, void* stream);
int h2_poseidon_merkle_device(h2_curve_t curve, uint32_t r_f, uint32_t r_p, const void* d_leaves, uint32_t depth, void* d_nodes,
                              void* stream);
int h2_poseidon_merkle_tail(void);      /* host only */
/* ---- a resident Poseidon Merkle tree: membership paths, batch verification, in-place update ------------------------
 * The tree is h2_poseidon_merkle_device's: d_leaves holds 2^depth elements, d_nodes the 2^depth - 1 inner nodes, level by
 * level from the leaves' parents up, the root last.  Elements are 4 x u64 Montgomery limbs; indices are uint32_t.  A path is
 * `depth` elements, the leaf's sibling first, then the sibling of every ancestor below the root.  Every call reports
 * per-item trouble in one uint32_t status word per item (H2_MERKLE_*), never as a host error.
 *   h2_poseidon_merkle_paths_device    a gather, no hashing: d_paths[i * depth + l] = the sibling at level l of leaf
 *                                      d_indices[i].  An index >= 2^depth gives status 1 and an all-zero path.
 *   h2_poseidon_merkle_verify_device   cur = d_leaf_values[i]; for every level l, cur = H(sib, cur) if bit l of the index is
 *                                      set, else H(cur, sib), H = ConstantLength<2> as in the tree.  d_roots_out[i] (optional)
 *                                      = the computed root.  Status 0 when the index is below 2^depth, the leaf value and
 *                                      every sibling are canonical and the computed root equals *d_root; d_root = NULL drops
 *                                      the comparison.  The data is untrusted: an element that is not canonical is never
 *                                      reduced silently -- status 2 and a zero root, as an index out of range (status 1) --
 *                                      and a root that differs is status 4.  The first that applies of 1, 2, 4 is reported.
 *                                      One path runs on the four lanes of a DPP quad (the permutation's three words side by
 *                                      side) or, in large batches, on one lane; the results are the same bits.
 *   h2_poseidon_merkle_update_device   afterwards d_leaves[d_indices[i]] = d_values[i] for the accepted items and d_nodes is
 *                                      byte for byte what h2_poseidon_merkle_device returns for the new leaves.  Items with
 *                                      status 1 (index) or 2 (value not canonical) are dropped first; of the remaining items
 *                                      with one index the LAST in the array is stored, the earlier ones get status 3.  Only
 *                                      the nodes above a stored leaf are hashed and written, everything else keeps its bytes.
 *                                      The tree must be consistent on entry (nodes = the hashes of the leaves).  Scratch:
 *                                      16 bytes per item and the sort's buffers, from the context's scan arena for the
 *                                      length of the call.
 * Asynchronous on `stream` under h2_ntt_device's rules: no host synchronisation and no device-to-host copy, except the first
 * use of a (curve, r_f, r_p) on a context, which uploads its constants as the calls above do.  H2_EINVAL -- checked on the host
 * before anything is enqueued -- for: an unknown curve; r_f odd or 0, or r_f + r_p > H2_POSEIDON_MAX_ROUNDS; depth = 0 or
 * depth > 30; n > 2^31; a null or not 16-byte aligned pointer (d_root and d_roots_out may be null, not misaligned); a range
 * that is written overlapping a range that is read or another that is written (the update's d_leaves and d_nodes count as
 * written).  n = 0 is H2_OK and enqueues nothing.  H2_ENOTINIT before h2_init.  h2_version() is unchanged: a host detects
 * these entry points by their symbols. */
#define H2_MERKLE_OK 0            /* the item is fine */
#define H2_MERKLE_RANGE 1         /* index >= 2^depth */
#define H2_MERKLE_NONCANONICAL 2  /* an element of the item is not below p */
#define H2_MERKLE_SUPERSEDED 3    /* update only: a later item writes the same leaf */
#define H2_MERKLE_MISMATCH 4      /* verify only: the computed root is not *d_root */
int h2_poseidon_merkle_paths_device(h2_curve_t curve, const void* d_leaves, const void* d_nodes, uint32_t depth,
                                    const void* d_indices, size_t n, void* d_paths /* n*depth */, void* d_status /* n */,
                                    void* stream);
int h2_poseidon_merkle_verify_device(h2_curve_t curve, uint32_t r_f, uint32_t r_p, const void* d_leaf_values /* n */,
                                     const void* d_indices, const void* d_paths, uint32_t depth, size_t n,
                                     const void* d_root /* 1 element or NULL */, void* d_roots_out /* n or NULL */,
                                     void* d_status /* n */, void* stream);
int h2_poseidon_merkle_update_device(h2_curve_t curve, uint32_t r_f, uint32_t r_p, void* d_leaves, void* d_nodes,
                                     uint32_t depth, const void* d_indices, const void* d_values /* n */, size_t n,
                                     void* d_status /* n */, void* stream);
/* ---- Poseidon at widths 3, 5 and 9: 4-ary and 8-ary hashes and Merkle trees ---------------------------------------
 * The same primitive (primitives.rs's Spec<F, T, RATE>) with the width as an argument: `width` = 3, 5 or 9, rate = width - 1
 * = 2, 4 or 8, S-box x^5, constants from the same Grain / Cauchy-MDS generation with t = width, over the scalar field of
 * `curve` (all three curves).  Width 3 is the family above, bit for bit (its calls are these at width 3); widths 5 and 9 are the two
 * the Poseidon paper proposes for Merkle trees of arity a = width - 1 = 4 and 8.  The caller supplies (r_f, r_p) under the
 * rules above; the library picks none.  The Poseidon paper's parameter script gives (8, 60) at t = 5 and (8, 63) at t = 9
 * for 128-bit security with x^5 on fields of about 255 bits -- NOT checked here: choosing round numbers is the caller's.
 * Elements are 4 x u64 Montgomery limbs, canonical; indices and status words are uint32_t, the status words H2_MERKLE_*.
 *   h2_poseidon_wide_constants            host only, no device and no h2_init needed: (r_f + r_p) * width round constants,
 *                                         then the width x width MDS row-major.  *n_elems = the elements that takes, also
 *                                         when cap_elems is too small.  At width 3: h2_poseidon_constants' elements.
 *   h2_poseidon_wide_permute_device       n states of `width` elements -> n states; d_out may be d_in exactly, otherwise
 *                                         the two must not overlap.
 *   h2_poseidon_wide_hash_device          ConstantLength<len> at rate width - 1: n messages of len elements, msg_stride
 *                                         elements apart, -> n elements.  The state starts as (0, .., 0, len 2^64), the
 *                                         capacity word LAST; `rate` words are absorbed per permutation, zero-padded; the
 *                                         output is word 0.
 *   h2_poseidon_wide_merkle_device        a^depth leaves -> the (a^depth - 1) / (a - 1) inner nodes, level by level from
 *                                         the leaves' parents up, the root last; a node is ConstantLength<a> of its a
 *                                         children in order.  Levels of more than h2_poseidon_merkle_tail() nodes take one
 *                                         launch each, all the levels above them one launch of a single workgroup.
 *   h2_poseidon_wide_merkle_paths_device  a gather, no hashing.  A path is depth * (a - 1) elements: at level l the a - 1
 *                                         siblings of the leaf's ancestor in child order, the ancestor's own position
 *                                         ((index / a^l) mod a) left out.  An index >= a^depth gives status 1 and an
 *                                         all-zero path.
 *   h2_poseidon_wide_merkle_verify_device cur = d_leaf_values[i]; at every level cur is inserted at its position among the
 *                                         level's siblings and the a words are hashed.  d_roots_out[i] (optional) = the
 *                                         computed root.  The rules of h2_poseidon_merkle_verify_device: untrusted data; an
 *                                         element that is not canonical is never reduced silently -- status 2 and a zero
 *                                         root, as an index out of range (status 1); another root than *d_root is status 4;
 *                                         the first that applies of 1, 2, 4 is reported; d_root = NULL drops the comparison.
 *                                         One path runs on one lane (width 3: or on four, as above).
 * There is no in-place update of a wide tree and no form with several lanes per permutation.
 * Asynchronous on `stream` under h2_ntt_device's rules, on the context of the calling thread's current HIP device; the first
 * use of a (curve, width, r_f, r_p) on a context builds and uploads its table and waits for that (the eight tables used last
 * are kept; a width-3 table is shared with the family above).  H2_EINVAL -- checked on the host before anything is enqueued
 * -- for: an unknown curve; a width other than 3, 5, 9; r_f odd or 0, or r_f + r_p > H2_POSEIDON_MAX_ROUNDS; a null or not
 * 16-byte aligned device pointer (d_root and d_roots_out may be null, not misaligned); len = 0 or len > 65535; msg_stride
 * < len or > 2^32; n > 2^40 (permute, hash) or 2^31 (paths, verify); depth = 0 or a^depth > 2^30; a range that is written
 * overlapping one that is read or another that is written (other than d_out == d_in of the permutation).  n = 0 is H2_OK
 * and enqueues nothing.  H2_ENOTINIT before h2_init.  h2_version() is unchanged: a host detects these entry points by their
 * symbols. */
int h2_poseidon_wide_constants(h2_curve_t curve, uint32_t width, uint32_t r_f, uint32_t r_p, uint64_t* out, size_t cap_elems,
                               size_t* n_elems);
int h2_poseidon_wide_permute_device(h2_curve_t curve, uint32_t width, uint32_t r_f, uint32_t r_p, const void* d_in, void* d_out,
                                    size_t n, void* stream);
int h2_poseidon_wide_hash_device(h2_curve_t curve, uint32_t width, uint32_t r_f, uint32_t r_p, const void* d_msgs, size_t len,
                                 size_t msg_stride, size_t n, void* d_out, void* stream);
int h2_poseidon_wide_merkle_device(h2_curve_t curve, uint32_t width, uint32_t r_f, uint32_t r_p, const void* d_leaves,
                                   uint32_t depth, void* d_nodes, void* stream);
int h2_poseidon_wide_merkle_paths_device(h2_curve_t curve, uint32_t width, const void* d_leaves, const void* d_nodes,
                                         uint32_t depth, const void* d_indices, size_t n,
                                         void* d_paths /* n*depth*(width-2) */, void* d_status /* n */, void* stream);
int h2_poseidon_wide_merkle_verify_device(h2_curve_t curve, uint32_t width, uint32_t r_f, uint32_t r_p,
                                          const void* d_leaf_values /* n */, const void* d_indices, const void* d_paths,
                                          uint32_t depth, size_t n, const void* d_root /* 1 element or NULL */,
                                          void* d_roots_out /* n or NULL */, void* d_status /* n */, void* stream);
/* ---- the lookup argument's permute and product steps over resident columns -----------------------------------
 * m lookups per call (those of one proof or of a batch).  Every column array holds m columns, col_stride elements apart,
 * over the scalar field of `curve` (all three curves), in the API form: 4 x u64 Montgomery limbs, canonical.  The ORDER
 * of field elements is that of their canonical integer value (`Ord` of halo2curves' Fr), not that of the limbs.
 * Both calls are asynchronous on `stream` under h2_ntt_device's rules and act on the context of the calling thread's
 * current HIP device, as h2_poly_eval_device does.  u = usable_rows (halo2: n - (blinding_factors + 1)); the blinding
 * rows [u, n) are the caller's, as with h2_poly_prefix_product_device.
 *
 * h2_lookup_permute_device: halo2_proofs src/plonk/lookup/prover.rs `permute_expression_pair(A, S)` over rows [0, u):
 *   A' = A[0..u] sorted ascending; left = sorted map value -> count over S[0..u]; S' = u zeros; rep = [];
 *   for row in 0..u: if row == 0 or A'[row] != A'[row-1] { S'[row] = A'[row]; left has no such value: the pair FAILS
 *   (Error::ConstraintSystemFailure), else its count drops by one } else rep.push(row);
 *   for (value, count) of left in ascending order, count times: S'[rep.pop()] = value   (pop from the END: the smallest
 *   leftover value lands on the largest repeated row).  Equal keys are indistinguishable, so A' and S' are unique.
 * Out of place: rows [0, u) of d_permuted_input (A') and d_permuted_table (S') are written, rows [u, col_stride) are not
 * touched.  d_status: m uint32 words of device memory, 0 = done, 1 = some input value is not in the table; for such a
 * pair d_permuted_input is still the full sorted column and the u rows of d_permuted_table are unspecified, the other
 * pairs are unaffected.  No host synchronisation: the caller reads the words when it wants them.
 * The columns are de-Montgomerised once and sorted by an LSD radix sort of 8-bit digits over the canonical 256-bit keys,
 * T = h2_lookup_tile() rows per workgroup and pass.  A digit on which all keys of a column agree is skipped; which of the
 * 32 passes run is decided ON THE DEVICE from the AND and OR of the keys (every pass is enqueued, a skipped one returns
 * at once), so nothing is read back and the call never waits: an 8-bit range table costs one or two passes, a
 * theta-compressed column up to 32.  Then each first occurrence binary-searches the sorted table, two scans rank the
 * repeated rows and the remaining table entries, and a scatter fills the repeated rows; outputs are re-Montgomerised.
 * Inputs that are not canonical give an unspecified order, never an out-of-range access: every index is formed from
 * usable_rows, m and bounded digit, rank or search values, and the launch geometry is proven on the host before anything
 * is enqueued (H2_EDEVICE with the violated condition in h2_last_device_error otherwise).
 * Scratch is the stream's MSM workspace for the length of the call (as h2_g_to_lagrange_device); nothing is cached or
 * kept.  One lookup needs about 136 * u bytes; a wide m runs in groups on `stream` so that the scratch stays under
 * max(1 GiB, what one lookup needs) and a group stays under 32767 lookups.
 *
 * h2_lookup_product_device: `commit_product` per lookup: z[0] = 1, z[i+1] = z[i] (A[i] + beta)(S[i] + gamma) /
 * ((A'[i] + beta)(S'[i] + gamma)) for i < u.  Rows [0, u] of every d_z column are written (z[u] = 1 for a satisfied
 * lookup), rows beyond are not touched; col_stride >= u + 1.  A zero denominator gives ratio 0 (batch_invert leaves zero
 * at zero).  One kernel writes the ratios (one inversion per run of 4 rows), the batched running product of
 * h2_poly_prefix_product_device follows in place.  beta, gamma: 4 Montgomery limbs each, host memory, read before return.
 *
 * H2_EINVAL, before anything is enqueued, for: an unknown curve; usable_rows > 2^26; col_stride < usable_rows (product:
 * < usable_rows + 1) or m * col_stride > 2^57; a device pointer that is not 16-byte aligned (d_status: 4-byte); with
 * m > 0 a null d_status / d_z / beta / gamma, and with m > 0 and usable_rows > 0 any other null pointer; permute: an
 * output range (d_status included) that overlaps an input range or another output; product: d_z overlapping a source.
 * H2_ENOTINIT before h2_init.  m = 0: H2_OK, nothing enqueued.  usable_rows = 0: permute writes m zero status words,
 * product writes z[0] = 1.
 * h2_version() did not change for these entry points: a host detects them by their symbols. */
int h2_lookup_permute_device(h2_curve_t curve, const void* d_input, const void* d_table, size_t usable_rows,
                             size_t col_stride, size_t m, void* d_permuted_input, void* d_permuted_table,
                             void* d_status, void* stream);
int h2_lookup_product_device(h2_curve_t curve, const void* d_input, const void* d_table, const void* d_permuted_input,
                             const void* d_permuted_table, size_t usable_rows, size_t col_stride, size_t m,
                             const uint64_t beta[4], const uint64_t gamma[4], void* d_z, void* stream);
/* rows one workgroup handles per sort pass (T above).  Host only, no h2_init needed: tests size their shapes by it. */
int h2_lookup_tile(void);
/* ---- the permutation argument's grand products over resident columns, chained on the device ------------------------
 * halo2_proofs src/plonk/permutation/prover.rs `Argument::commit` for m instances (the proofs of a batch) in one call,
 * over the scalar field of `curve` (all three curves), columns in the API form: 4 x u64 Montgomery limbs, canonical.
 * u = usable_rows (halo2: n - (blinding_factors + 1)); the n_cols permutation columns are cut into S = ceil(n_cols /
 * chunk_len) sets, set s holding the columns j in [s chunk_len, min((s + 1) chunk_len, n_cols)) (halo2: chunk_len =
 * cs.degree() - 2).  Per instance, with its own beta and gamma:
 *   ratio_s[i] = prod_{j in set s} (v_j[i] + beta delta^j omega^i + gamma)
 *              / prod_{j in set s} (v_j[i] + beta sigma_j[i]      + gamma)        for i < u
 *   z_0[0] = 1;   z_s[i+1] = z_s[i] ratio_s[i]  for i < u;   z_{s+1}[0] = z_s[u]
 * j is the column's index among ALL n_cols columns, not its position within the set.  A row whose denominator is zero has
 * ratio 0 (batch_invert leaves zero at zero): every later row of that instance, in that set and in all later sets, is
 * then 0; other instances are unaffected.
 * d_values: HOST array of m * n_cols device pointers, column j of instance p at [p * n_cols + j]; d_sigma: HOST array of
 * n_cols device pointers, the key's permutation columns in Lagrange form, shared by the instances.  Every source column
 * has u readable rows and is 16-byte aligned; pointers may repeat, within an instance and across instances.  beta, gamma:
 * HOST, m * 4 limbs each (one pair per instance); omega (the domain's generator), delta: HOST, 4 limbs.  All host arrays
 * are read before the call returns.
 * d_z: m * S output columns, column p * S + s col_stride elements after the previous one.  Rows [0, u] of every column
 * are written, canonical; rows (u, col_stride) are NOT touched: they are the caller's blinding rows (and the RNG draws
 * that fill them stay the caller's), as with h2_lookup_product_device.  z_{S-1}[u] = 1 when the copy constraints hold.
 * Asynchronous on `stream` under h2_ntt_device's rules, on the context of the calling thread's current HIP device.  No
 * host synchronisation and no device-to-host copy anywhere in the call: set s + 1 starts at the last usable value of set
 * s, so the S columns of an instance are ONE running product over the sequence (set, row), and one scan that walks the
 * sets in order carries the tail across them.  Four launches whatever S and n_cols are: one ratio kernel (grid: tiles of
 * T = h2_permutation_tile() rows x S x instances; arguments -- the pointers and beta delta^j, prepared once per instance
 * and column on the host -- from a table in HBM, so any chunk length is allowed; one Fermat inversion per run of 4 rows;
 * omega^i from a table of the 25 powers omega^(4 2^b)), then the three launches of h2_poly_prefix_product_device's scan
 * with element e of an instance at column e / u, row e % u, in place; the value at a set boundary also lands in row u
 * of the set before.  The ratio kernel takes up to 65535 instances per launch, the scan 256; a wider m runs in groups on
 * `stream`.  Results are the same bits whatever m is and however instances are grouped.
 * Scratch comes from the context's scan arena for the length of the call: the argument table (48 bytes per instance and
 * column, 64 per instance), the power table (800 bytes) and the scan's chunk values (256 KiB per instance of a group).
 * Nothing is cached or kept.  The launch geometry is proven on the host before anything is enqueued (H2_EDEVICE with the
 * violated condition in h2_last_device_error otherwise: S > 65535, m * n_cols > 2^32).
 * m = 0 or n_cols = 0: H2_OK, nothing enqueued, nothing written.  u = 0: z_s[0] = 1 for every column.
 * H2_EINVAL, before anything is enqueued, for: an unknown curve; chunk_len = 0 with n_cols > 0; usable_rows > 2^26;
 * col_stride < usable_rows + 1; m * S * col_stride > 2^57; with m > 0 and n_cols > 0 a null host array, a null d_z or a
 * d_z that is not 16-byte aligned; with usable_rows > 0 additionally a null or misaligned entry of d_values or d_sigma,
 * or the d_z range overlapping rows [0, u) of any source column.  H2_ENOTINIT before h2_init.
 * h2_version() did not change for these entry points: a host detects them by their symbols. */
int h2_permutation_product_device(h2_curve_t curve, const void* const* d_values, const void* const* d_sigma, size_t n_cols,
                                  size_t chunk_len, size_t usable_rows, size_t m, const uint64_t* beta,
                                  const uint64_t* gamma, const uint64_t omega[4], const uint64_t delta[4], void* d_z,
                                  size_t col_stride, void* stream);
/* rows one workgroup of the ratio kernel covers (T above).  Host only, no h2_init needed: tests size their shapes by it. */
int h2_permutation_tile(void);
/* ---- expressions over resident columns: evaluate_h in one launch ---------------------------------------------------
 * A host hands over an expression DAG once (every gate, the permutation and lookup terms, folded by y) and evaluates it
 * on every row of the extended domain for m instances per call, over the scalar field of `curve` (all three curves).
 * The library compiles the DAG to a straight-line program -- shared subexpressions found, ordered to need few live
 * values, a product with one inserted where lazy magnitudes would grow too large -- and one kernel interprets it per row:
 * no scratch column, no pass over HBM per node.
 *
 * Nodes: op 0 constant number x | 1 column a at rotation x | 2 add, 3 sub, 4 mul of the EARLIER nodes a and b |
 * 5 variable number x.  The last node is the root.  halo2's Negated lowers to 0 - a, Scaled to a product with a
 * constant; challenges (y, beta, gamma, theta, beta delta^j) are variables, set per call and instance.  A root that is a
 * leaf is legal: the library multiplies it by one.
 *
 * h2_expr_compile: host only, needs neither h2_init nor a GPU, and does not recurse: a y-fold as deep as the DAG is long
 * compiles on a small thread stack.  consts: n_consts x 4 Montgomery limbs, canonical.  The
 * handle keeps the compiled code; every context gets a device copy at its first h2_expr_eval_device, freed by
 * h2_expr_release or h2_shutdown (the handle itself outlives h2_shutdown).  H2_EINVAL, with the violated rule in
 * h2_last_device_error, for: an unknown curve; a null pointer with a non-zero count; n_nodes = 0; n_nodes, n_consts
 * or n_vars above 2^20; an operand that is not an earlier node; an unknown op; a constant, column or variable index at or beyond
 * n_consts, n_cols, n_vars; n_cols > 2^22; a rotation outside [-128, 127]; a constant that is not canonical; a program
 * whose live values need more LDS than one workgroup may hold (75 values: split the DAG and pass the partial result as a
 * column of the next program).
 * h2_expr_info: the program's counters.  h2_expr_dump: the six counters instructions, products, column reads, slots,
 * constants, reductions (u32), the code (12 bytes per instruction), the constant table (32 canonical little-endian bytes
 * each, zero for a variable), then n_vars u32: the table index of each variable.  *out_len receives the length; H2_EINVAL
 * when cap is smaller.
 *
 * h2_expr_eval_device: for instance p < m and row i < 2^log_rows, out[p * out_stride + i] = the root's value, where
 * column c at rotation r reads d_cols[p * n_cols + c][(i + r * rot_step) mod 2^log_len[c]] and variable v is
 * vars[p * n_vars + v].  log_len[c] <= log_rows: a shorter column is periodic, as t_evaluations is.  With rot_step =
 * 2^(extended_k - k) on extended columns this is one evaluate_h.  Everything is in the API form (4 x u64 Montgomery
 * limbs); the output is canonical, written out of place, and has the same bits whatever m is.  d_cols (m * n_cols device
 * pointers), log_len (n_cols) and vars (m * n_vars * 4 limbs) are HOST arrays, read before the call returns.
 * Asynchronous on `stream` under h2_ntt_device's rules, on the context of the calling thread's current HIP device; the
 * pointer table and the constant tables of the instances live in that context's scratch for the length of the call, as
 * h2_poly_eval_device's job table does.  m > 65535 runs in groups on the same stream.
 * H2_EINVAL, before anything is enqueued, for: log_rows > 28; log_len[c] > log_rows; out_stride < 2^log_rows,
 * m > 2^30 or m * out_stride > 2^57; a null host array with a non-zero count; a null or not 16-byte aligned column pointer or d_out;
 * a variable that is not canonical; a column that overlaps rows that are written (rows [0, 2^log_rows) of any instance's
 * out_stride rows; a column inside the unwritten rows between two instances is fine).  H2_EHANDLE for an unknown handle,
 * H2_ENOTINIT before h2_init; m = 0: H2_OK, nothing enqueued.
 * Column CONTENTS are not checked: an element that is not canonical gives a wrong value, never an out-of-range access.
 * Every index is formed from the row, the instruction words -- whose constant, column and slot numbers were proven
 * against n_cols and the table sizes at compile time -- and log_len.
 * h2_version() did not change for these entry points: a host detects them by their symbols. */
typedef struct {
  int32_t op, a, b, x;
} h2_expr_node_t;
typedef struct {
  uint32_t curve, instructions, products, column_reads, slots, constants, reductions, n_cols, n_vars, lds_bytes;
  int32_t min_rot, max_rot;
} h2_expr_info_t;
int h2_expr_compile(h2_curve_t curve, const h2_expr_node_t* nodes, size_t n_nodes, const uint64_t* consts, size_t n_consts,
                    uint32_t n_cols, uint32_t n_vars, uint64_t* handle_out);
int h2_expr_release(uint64_t handle);
int h2_expr_info(uint64_t handle, h2_expr_info_t* out);
int h2_expr_dump(uint64_t handle, uint8_t* out, size_t cap, size_t* out_len);
int h2_expr_eval_device(uint64_t handle, const void* const* d_cols, const uint32_t* log_len, const uint64_t* vars, size_t m,
                        uint32_t log_rows, uint32_t rot_step, void* d_out, size_t out_stride, void* stream);
/* out[i] = Scalar::random(rng) number first_block + i of rng = ChaCha20Rng::from_seed(seed), Montgomery limbs:
 * the coefficients of the vanishing argument's random_poly (halo2_proofs src/plonk/vanishing/prover.rs
 * `Argument::commit`).  Each draw consumes one 64-byte ChaCha20 block. */
int h2_chacha20_scalars_device(h2_curve_t curve, const uint8_t seed[32], uint64_t first_block, size_t n, void* d_out,
                               void* stream);

/* ---- introspection used by bench.py's roofline (no effect on results) --------------------
 * Names the kernels launched by the last h2_msm* / h2_ntt* call and their geometry. */
typedef struct {
  uint32_t window_bits;   /* c */
  uint32_t windows;       /* W */
  uint32_t buckets;       /* 2^(c-1) */
  uint64_t table_bytes;   /* resident precomputed table */
} h2_msm_plan_t;
int h2_msm_plan(uint64_t bases_handle, h2_msm_plan_t* out);


/* ---- best_fft over group elements ------------------------------------------------------------
 * Replaces halo2_proofs::arithmetic::best_fft<Scalar, G> for G = C::Curve (the FftGroup impl of the curve's projective
 * points): the reference's only use is ParamsKZG::new -> g_to_lagrange, reached from
 * /root/reference/circuits/src/utils.rs:59-61 (g_lagrange = n^-1 * best_fft(g, omega^-1, k)).  n = 2^log_n Jacobian
 * points (96 bytes, Montgomery limbs, identity z = 0) transformed IN PLACE, natural order in and out, unscaled, omega in
 * the scalar field's Montgomery form.  Results are group elements: compare after affine normalisation.
 * h2_fft_group: host pointer, synchronous; h2_fft_group_device: device pointer, asynchronous on `stream`. */
int h2_fft_group(h2_curve_t curve, uint64_t* points_jac, const uint64_t omega[4], uint32_t log_n);
int h2_fft_group_device(h2_curve_t curve, void* d_points_jac, const uint64_t omega[4], uint32_t log_n, void* stream);

/* ---- g_to_lagrange and Params::downsize: a Lagrange-basis SRS without the toxic scalar ---------------------
 * ParamsKZG::new's g_to_lagrange in one call: out[i] = [scale] sum_{j<n} [omega_inv^(i j)] g[j], n = 2^log_n,
 * affine in (64 B, identity (0,0)), affine out (normalised, canonical Montgomery limbs, identity (0,0)).
 * With omega_inv = omega^-1 of the 2^log_n domain and scale = n^-1 this is g_lagrange: it replaces best_fft over the
 * projective points, the n multiplications by n^-1 and batch_normalize.  scale = 1 skips the scaling; log_n = 0 copies
 * the point times scale.
 * h2_g_to_lagrange_device: device pointers, asynchronous on `stream` (NULL: the library's), on the calling thread's
 * current context; scratch is the stream's MSM workspace for the length of the call (as h2_fft_group_device), nothing is
 * cached.  d_out_affine may EQUAL d_g_affine (the points are read into the scratch first); a partial overlap of the two
 * n * 64-byte ranges is H2_EINVAL.  H2_EINVAL, before anything is enqueued, also for an unknown curve, a null pointer,
 * a device pointer that is not 16-byte aligned, or log_n > 26; H2_ENOTINIT before h2_init.
 * h2_g_to_lagrange: host pointers (out_affine may be g_affine), context 0, synchronous.
 * The points are NOT checked to be on the curve (best_fft does not check either): garbage in, garbage out, no fault;
 * h2_bases_register stays the checked route and checks the output when it is used.
 * h2_version() did not change for these entry points: a host detects them by their symbols. */
int h2_g_to_lagrange_device(h2_curve_t curve, const void* d_g_affine, uint32_t log_n, const uint64_t omega_inv[4],
                            const uint64_t scale[4], void* d_out_affine, void* stream);
int h2_g_to_lagrange(h2_curve_t curve, const uint64_t* g_affine /* n*8 */, uint32_t log_n, const uint64_t omega_inv[4],
                     const uint64_t scale[4], uint64_t* out_affine /* n*8 */);
/* Params::downsize(k) on the params wire format of h2_setup (BN254: u32 k, g, g_lagrange, 256 bytes of G2): the output
 * holds k, g[..2^k], g_to_lagrange of that prefix (omega^-1 and n^-1 of the 2^k domain) and the G2 tail copied.  k equal
 * to the blob's own k takes the same path and recomputes g_lagrange.  Synchronous, on the calling thread's current
 * context.  The blob is parsed as the prove and verify entry points parse it: H2_EPROOF for a truncated blob or a length
 * that is not its k's; H2_EINVAL for k < 1 or k above the blob's k (or above 26).  *out_len receives the output's length
 * (also when the call returns H2_EINVAL because `out` is null or cap is too small, as h2_setup).  Nothing is registered
 * and the params cache is not touched: the points are validated when the output is later used as params. */
int h2_params_downsize(const uint8_t* params, size_t params_len, uint32_t k, uint8_t* out, size_t cap, size_t* out_len);

/* ---- SRS generation == the g vector of ParamsKZG::new(k) -----------------------------------
 * d_out_affine[i] = [s^i] G for i < n (device memory, n*64 bytes), s in Montgomery form.
 * Counterpart of the setup loop reached from /root/reference/circuits/src/utils.rs:59-61 and
 * wasm.rs:49-55; also how bench.py makes valid synthetic bases without the CPU oracle. */
int h2_srs_generate(h2_curve_t curve, const uint64_t s[4], size_t n, void* d_out_affine, void* stream);

/* d_out_affine[i] = [k_i] G for n scalars in device memory (Montgomery form): with k_i = L_i(s), the Lagrange
 * basis at the toxic scalar, this is the g_lagrange vector of ParamsKZG::new(k). */
int h2_fixed_base_mul(h2_curve_t curve, const void* d_scalars, size_t n, void* d_out_affine, void* stream);

/* ---- kernel timing for bench.py's roofline ---------------------------------------------------
 * While enabled, every MSM launch records HIP events (on the launch stream) around its
 * bucket-accumulate kernel.  h2_profile_read waits for them, returns the sums and resets. */
typedef struct {
  uint64_t launches;         /* accumulate-kernel launches timed */
  double kernel_ms;          /* sum of their durations */
  double algorithmic_bytes;  /* sum over launches of m*n*(32+64) + m*96 */
} h2_profile_t;
int h2_profile_enable(int on);
int h2_profile_read(h2_profile_t* out);

/* ---- the product surface: setup / prove / verify / simulate / count -----------------------------------
 * C counterparts of the reference's five wasm-bindgen exports (/root/reference/circuits/src/wasm.rs:49 setup,
 * :68 wasm_simulate_circuit, :77 wasm_generate_proof, :125 wasm_verify_proof, :182 get_circuit_count), i.e. of
 * utils.rs:59-158 (generate_params, generate_keys, generate_proof[_with_instance], verify[_with_instance]) over
 * KZG / BN254 with a Blake2b transcript: circuit 0 = Collatz (SHPLONK, no instance), 1 = arithmetic (GWC, public
 * inputs [constant, z]), anything else = Poseidon (GWC; prove takes hex_to_fr(output), verify recomputes the hash
 * of x).  Params and proofs use the reference's wire formats, so artefacts interoperate.
 * Everything numeric runs on the GPU of the current context; the SRS tables of the last few distinct params blobs
 * stay registered between calls.
 *
 * Randomness comes from the caller, call by call as the reference's RngCore is used: Fr::random = eight calls of
 * 8 bytes, the blinding polynomial's ChaCha20 seed = one call of 32 bytes.  rng = NULL draws from the OS.  With
 * the same stream the proof bytes equal the reference's.
 *
 * Output buffers are caller-owned; *out_len receives the size (also when the call returns H2_EINVAL because
 * `cap` is too small).  Malformed params / JSON / proofs give H2_EPROOF (the reference panics); a well-formed
 * proof that does not verify is *ok = 0 with H2_OK (the reference traps for the GWC circuits, utils.rs:150-157). */
typedef void (*h2_rng_fill_t)(void* ctx, uint8_t* out, size_t n);
int h2_setup(uint32_t k, h2_rng_fill_t rng, void* rng_ctx, uint8_t* out, size_t cap, size_t* out_len);
int h2_generate_proof(const uint8_t* params, size_t params_len, const char* json, int circuit, h2_rng_fill_t rng,
                      void* rng_ctx, uint8_t* out, size_t cap, size_t* out_len);
/* `count` proofs of ONE circuit under ONE params blob, each from its own JSON input, made in lockstep: every commit
 * phase, transform and read-back is issued once for the batch (in groups of 16 proofs up to k = 16, half as many with every step of k above
 * that), not once per proof.  Proof i is
 * byte for byte what h2_generate_proof(params, jsons[i], circuit, rng, rng_ctxs[i]) returns: proof i draws only through
 * rng(rng_ctxs[i], ...), in h2_generate_proof's order.  rng = NULL: the OS.  rng_ctxs = NULL: every proof passes a NULL
 * context (the order of draws BETWEEN proofs is then unspecified; within a proof it is h2_generate_proof's).
 * The proofs are written back to back into `out`; proof_lens[i] (count entries, required when count > 0) receives each
 * length, *out_len the total (also when the call returns H2_EINVAL because cap is too small).  All or nothing: every
 * JSON is parsed and every witness synthesised before anything is enqueued; a bad item gives the status h2_generate_proof
 * gives for it and `out` is not written.  count = 0: H2_OK, *out_len = 0.  h2_version() is unchanged by this entry
 * point: a caller detects it by the symbol. */
int h2_generate_proofs(const uint8_t* params, size_t params_len, size_t count, const char* const* jsons, int circuit,
                       h2_rng_fill_t rng, void* const* rng_ctxs, uint8_t* out, size_t cap, size_t* proof_lens,
                       size_t* out_len);
int h2_verify_proof(const uint8_t* params, size_t params_len, const uint8_t* proof, size_t proof_len,
                    const char* json, int circuit, int* ok);
/* `count` proofs of ONE circuit under ONE params blob, each with its own JSON input (upstream halo2's
 * plonk::BatchVerifier).  ok[i] (count ints, required) receives exactly what h2_verify_proof would have written for
 * proof i; *all_ok (optional) = 1 iff every ok[i] is 1 (count = 0: H2_OK, *all_ok = 1).  The transcripts are replayed on
 * the host one by one -- their compressed points decompressed beforehand by one kernel launch for the whole batch -- and
 * the N final checks e(L_i, [s]G2) e(R_i, -G2) = 1 collapse into e(sum r_i L_i, [s]G2) e(sum r_i R_i, -G2) = 1: one small
 * MSM launch and one pairing for up to 1024 proofs, which a batch holding a bad proof passes with probability at most
 * 2^-128.  When it fails the batch is halved until the culprits are found (about 2 log2 N further checks per bad proof).
 * rng supplies the weights r_i (16 bytes per proof, read little-endian; NULL = the OS); a zero weight is never used.
 * The weights must be unpredictable to whoever made the proofs.  H2_EPROOF / H2_EINVAL under the same conditions as
 * h2_verify_proof, for any item (a NULL ok, proofs, proof_lens or jsons with count > 0: H2_EINVAL). */
int h2_verify_proofs(const uint8_t* params, size_t params_len, size_t count, const uint8_t* const* proofs,
                     const size_t* proof_lens, const char* const* jsons, int circuit, h2_rng_fill_t rng, void* rng_ctx,
                     int* ok, int* all_ok);
/* the NUL-terminated result string of wasm_simulate_circuit ("N/A" for Collatz) */
int h2_simulate(const char* json, int circuit, char* out, size_t cap, size_t* out_len);
int h2_circuit_count(void);
/* The SRS of the last few distinct params blobs stays registered (MSM tables resident in HBM) between calls; this
 * releases them: the next call parses and registers its params again, as the reference does on every call. */
int h2_params_cache_clear(void);
/* Proving keys (fixed + permutation columns in all their forms, their commitments, the vk digest, the compiled
 * quotient program) depend only on the params and the circuit index; the reference rebuilds them on every prove and
 * verify call (wasm.rs:86,95,114,132), this library keeps them by default.  h2_key_cache(0) restores the
 * reference's behaviour (bench.py times both); returns the previous setting. */
int h2_key_cache(int enable);

/* ---- the IPA batch verifier on the Pasta curves -------------------------------------------------------------------
 * verify_proof of the inner product argument (poly/ipa/commitment/verifier.rs) for `count` proofs behind combined checks,
 * in ONE call: between the upload of the proofs and the 96-byte read-back of each combined check nothing goes through the
 * host but the random weights.  DESIGN.md section 7.17.
 *
 * A transcript midstate.  The device has to start where the caller's transcript stands, so the Blake2b state crosses the
 * ABI as a plain struct: the chaining words, the bytes compressed so far, the block buffer (bytes behind buflen zero) and
 * buflen, 0 .. 128 -- Blake2b keeps a FULL buffer uncompressed until more input arrives, because the last block is
 * finalised with a flag.  Host only, no h2_init needed:
 *   h2_transcript_init        the personalised "Halo2-Transcript" state with a 64-byte digest, nothing absorbed
 *   h2_transcript_absorb      len bytes (common_point: 0x01 || x || y, common_scalar: 0x02 || s, canonical little-endian)
 *   h2_transcript_challenge   squeeze_challenge: absorbs 0x00, finalises a COPY and reduces the 64 bytes modulo the scalar
 *                             field of `curve` (any of the three): out = 4 Montgomery limbs.  The state keeps absorbing.
 * H2_EINVAL for a null pointer, an unknown curve or a state whose buflen is above 128. */
typedef struct {
  uint64_t h[8];        /* chaining words */
  uint64_t t;           /* bytes compressed so far (the buffer's not included) */
  uint8_t buf[128];     /* block buffer */
  uint32_t buflen;      /* 0 .. 128 */
  uint32_t reserved;    /* 0 */
} h2_transcript_state_t; /* 208 bytes */
int h2_transcript_init(h2_transcript_state_t* state);
int h2_transcript_absorb(h2_transcript_state_t* state, const uint8_t* bytes, size_t len);
int h2_transcript_challenge(h2_curve_t curve, h2_transcript_state_t* state, uint64_t out[4]);
/* The transcripts of `count` proofs of one k, one lane each, in upstream's order: absorb S, squeeze xi and z, k times absorb
 * L_j and R_j and squeeze u_j, absorb c and f.  A point is absorbed as 0x01 || x || y, the identity (point status 2) as 64
 * zero bytes behind the 0x01, as common_point does.
 *   d_states        count x 208 bytes, the midstate each proof's transcript starts from (a buflen above 128 is read as 128)
 *   d_points        count x (2k + 1) affine points of 64 bytes, S, L_0, R_0, L_1, ...: h2_pasta_points_decompress_device's output
 *   d_point_status  count x (2k + 1) bytes: that call's status
 *   d_scalars       count x 64 bytes: c || f as they stand in the stream
 *   d_out           count x (k + 4) x 32 bytes: xi, z, u_0 .. u_(k-1), c, f as Montgomery limbs
 *   d_status        count bytes, the first that applies: 1 a point of decompression status 1 or 3; 2 c or f not canonical;
 *                   3 some u_j = 0; 0 otherwise.  The d_out row of a proof with a status other than 0 is unspecified.
 *   d_states_out    null, or count x 208 bytes: the midstates behind f
 * Asynchronous on `stream`, no host synchronisation, nothing allocated.  H2_EINVAL, before anything is enqueued, for
 * H2_BN254 (the wire form is the Pasta one) or an unknown curve, k = 0, k > H2_IPA_MAX_K, count > 2^24; count = 0 is H2_OK
 * whatever the pointers; otherwise a null pointer other than d_states_out, or one of d_states, d_points, d_scalars, d_out,
 * d_states_out that is not 16-byte aligned, is H2_EINVAL. */
int h2_ipa_replay_device(h2_curve_t curve, uint32_t k, size_t count, const void* d_states, const void* d_points,
                         const void* d_point_status, const void* d_scalars, void* d_out, void* d_status, void* d_states_out,
                         void* stream);
/* The batch verifier.  `bases` is the handle of G || U || W (2^k + 2 points) the h2_ipa_* calls take.  Item i: the midstate
 * states[i] its transcript stands at, its proof bytes, the commitment (8 Montgomery limbs, affine, (0, 0) the identity), x3
 * and v (4 canonical Montgomery limbs each); all HOST arrays.  ok[i] (count ints) is exactly what verify_proof gives for the
 * item; *all_ok (optional) is their AND (count = 0: 1); *checks_out (optional) the combined checks that ran.
 * A proof is exactly (2k + 3) * 32 bytes -- S, k x (L_j, R_j), c, f.  Any other length is ok[i] = 0 without a device step: a
 * shorter stream fails verify_proof's reads, and bytes behind the proof belong to the caller's transcript, so the caller
 * passes the proof's own length.
 * One upload, one decompression launch and one replay launch for the batch; one read-back of the status bytes decides
 * which proofs take part.  A combined check draws 16 bytes per proof of its subset from rng, in subset order, read
 * little-endian, a zero weight redrawn (rng = NULL: the OS; the weights must be unpredictable to whoever made the proofs),
 * makes the scalars on the device, runs the challenge-product sum, one MSM on the registered table, one over the
 * decompressed points with the commitments behind them, and reads 96 bytes back.  A failing subset is halved until every
 * culprit is alone.  Synchronous, on the context's stream; scratch comes from the context's arenas.
 * H2_EINVAL for H2_BN254 or an unknown curve, k = 0 or k > H2_IPA_MAX_K, a handle of another curve or one that does not hold
 * exactly 2^k + 2 bases (H2_EHANDLE for one that is not registered), a null array with count > 0, a null proof of non-zero
 * length, an x3 or v that is not canonical, a state whose buflen is above 128. */
int h2_ipa_verify_proofs(h2_curve_t curve, uint64_t bases, uint32_t k, size_t count, const h2_transcript_state_t* states,
                         const uint8_t* const* proofs, const size_t* proof_lens, const uint64_t* commitments, const uint64_t* x3,
                         const uint64_t* v, h2_rng_fill_t rng, void* rng_ctx, int* ok, int* all_ok, size_t* checks_out);

/* ---- the IPA prover behind one call, on the Pasta curves -----------------------------------------------------------
 * create_proof of the inner product argument (poly/ipa/commitment/prover.rs) for m openings of one k in lockstep with the
 * transcripts on the device: behind every round's MSM one lane per opening writes L_j, R_j in the wire form, absorbs them,
 * squeezes u_j, inverts it and writes the scalars of the next round, so from round 0 to f nothing goes through the host.
 * DESIGN.md section 7.20.  h2_version() did not change for these entry points, it stays 1002: a host detects them by their
 * symbols.
 *
 * h2_ipa_prove_state_bytes: host only, no h2_init needed.  The size of the state h2_ipa_prove_rounds_device works in: its
 * first h2_ipa_batch_state_bytes(k, m) bytes are that call's state, unchanged; behind them what the route keeps resident --
 * every blind, f, the midstates, the rounds' points.  A multiple of 16.  H2_EINVAL for k = 0, k > H2_IPA_MAX_K, m = 0,
 * m > H2_IPA_MAX_BATCH or a null out.
 *
 * h2_ipa_prove_rounds_device: begin, k rounds and final of h2_ipa_*_batch_device with the transcript step behind each.
 *   d_p           HOST array of m device pointers: p'_i, 2^k coefficients each, only read
 *   x3, z, f0     m x 4 limbs each: the opening points, the challenges z_i, and f_i as it stands, s_blind_i xi_i + p_blind_i
 *   round_blinds  m x 2k x 4 limbs: l_0, r_0, l_1, r_1, ... of opening i
 *   states        m midstates: each transcript where it stands behind the two challenges squeezed after S
 *   d_state       h2_ipa_prove_state_bytes(k, m) bytes, 16-byte aligned; what an earlier use left in it does not matter
 *   d_tail        m x (2k + 2) x 32 bytes, 16-byte aligned: L_0, R_0, ..., L_(k-1), R_(k-1), c, f of opening i in the wire form
 *   d_states_out  null, or m x 208 bytes, 16-byte aligned: the midstates behind f
 *   d_status      m x uint32_t: 0, or 1 when some challenge u_j of the opening was zero -- its 1 / u_j is then taken as zero,
 *                 nothing traps, and the opening's bytes in d_tail are unspecified
 * All scalars are canonical Montgomery limbs.  Asynchronous on `stream` under h2_ntt_device's rules; the host arrays are read
 * before the call returns.  ONE upload in front of the kernels; after it no host synchronisation and no device-to-host copy.
 * Every round's MSM goes through the registered table's own launch path with its bounds proof, and what that path refuses
 * is found before anything is enqueued.  No device memory is allocated beyond the context's MSM workspace.
 * H2_EINVAL, before anything is enqueued, for H2_BN254 (the wire form is the Pasta one) or an unknown curve, k = 0,
 * k > H2_IPA_MAX_K, m = 0, m > H2_IPA_MAX_BATCH, a null array, a null or misaligned device pointer (every d_p[i] included;
 * d_status 4-byte aligned), a scalar that is not canonical, a state whose buflen is above 128, a handle of another curve or
 * one that does not hold exactly 2^k + 2 bases (H2_EHANDLE for one that is not registered).
 *
 * h2_ipa_create_proofs: upstream's create_proof for m openings with EVERY random value supplied by the caller, so the bytes
 * are a function of the arguments.  The blinds and the seeds must be uniform and secret: they are what hides the polynomials.
 *   states        where each item's transcript stands before S
 *   d_p, p_blind  HOST array of m device pointers to the polynomials (2^k coefficients, only read); their blinds
 *   d_s_poly      HOST array of m device pointers to the blinding polynomials (only read); entry i null: s_poly_i is
 *                 expanded from the 32 bytes at seeds + 32 i as h2_chacha20_scalars_device expands them from block 0
 *   seeds         m x 32 bytes; may be null when no d_s_poly entry is null
 *   s_blind       m x 4 limbs; round_blinds as above
 *   proofs        m x (2k + 3) x 32 bytes: S, k x (L_j, R_j), c, f -- what h2_ipa_verify_proofs takes
 *   states_out    null, or m midstates behind f;  status: m words, as d_status above
 * The preamble -- the 2 m evaluations, s_poly_i[0] -= s_poly_i(x3_i), the m commitments S_i as one MSM, S absorbed and xi, z
 * squeezed on the host, p'_i = xi_i s_poly_i + p_i with p'_i[0] -= p_i(x3_i) -- then h2_ipa_prove_rounds_device's work, then one
 * read-back.  Three stream synchronisations per call whatever k and m are: behind the evaluations, behind S, at the end.
 * Synchronous, on the context's stream; scratch comes from the context's arenas.  H2_EINVAL as above, and for a null seeds
 * with a null d_s_poly entry. */
int h2_ipa_prove_state_bytes(uint32_t k, size_t m, size_t* out);
int h2_ipa_prove_rounds_device(h2_curve_t curve, uint64_t bases, uint32_t k, size_t m, const void* const* d_p, const uint64_t* x3,
                               const uint64_t* z, const uint64_t* f0, const uint64_t* round_blinds,
                               const h2_transcript_state_t* states, void* d_state, void* d_tail, void* d_states_out,
                               void* d_status, void* stream);
int h2_ipa_create_proofs(h2_curve_t curve, uint64_t bases, uint32_t k, size_t m, const h2_transcript_state_t* states,
                         const void* const* d_p, const uint64_t* p_blind, const uint64_t* x3, const void* const* d_s_poly,
                         const uint8_t* seeds, const uint64_t* s_blind, const uint64_t* round_blinds, uint8_t* proofs,
                         h2_transcript_state_t* states_out, uint32_t* status);

#ifdef __cplusplus
}
#endif
#endif /* H2HIP_H */
