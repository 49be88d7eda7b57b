// h2_selftest.hip -- the test hooks of include/h2hip_selftest.h that sit beside the drop-in C ABI (h2_capi.hip): the host and
// device instantiations of the field / curve / 29-bit templates, the MSM workspace checks and the test knobs.  Not a compute
// path; nothing here is called by the library itself.
#include "h2_internal.hpp"
#include "h2_field29_chain.hpp"
#include "h2_host.hpp"
#include "h2_ipa_prove.hpp"
#include "h2_poseidon.hpp"

#include <cstdio>
#include <vector>

#include "../../include/h2hip_selftest.h"

using namespace h2;

extern "C" int h2_selftest_field_op(int field, int op, const uint64_t a[4], const uint64_t b[4], uint64_t out[4]) {
  if (!a || !b || !out) return H2_EINVAL;
  int rc = -1;
  switch (field) {
    case 0: rc = curve_ops_bn254()->selftest_field(0, op, a, b, out); break;   // bn254 Fq
    case 1: rc = curve_ops_bn254()->selftest_field(1, op, a, b, out); break;   // bn254 Fr
    case 2: rc = curve_ops_pallas()->selftest_field(0, op, a, b, out); break;  // pasta Fp
    case 3: rc = curve_ops_pallas()->selftest_field(1, op, a, b, out); break;  // pasta Fq
  }
  return rc == 0 ? H2_OK : H2_EINVAL;
}
// one operand set (a, b, c, d: 9 limbs each) through op 0..3; the host hook and the device kernel run this same source
template <class FP>
H2_HD void selftest_fe29_run(int op, const int32_t* in, int32_t* out) {
  Fe29<FP> a[4];
  for (int k = 0; k < 4; k++)
    for (int l = 0; l < 9; l++) a[k].v[l] = in[9 * k + l];
  Fe29<FP> r;
  switch (op) {
    case 0: r = fe29_mul(a[0], a[1]); break;
    case 1: r = fe29_sqr(a[0]); break;
    case 2: r = fe29_mul_sub(a[0], a[1], a[2], a[3]); break;
    default: r = fe29_mul_up(a[0], a[1]); break;
  }
  for (int l = 0; l < 9; l++) out[l] = r.v[l];
}
template <class FP>
__global__ void __launch_bounds__(64) selftest_fe29_kernel(int op, const int32_t* __restrict__ in, int32_t* __restrict__ out,
                                                           uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  selftest_fe29_run<FP>(op, in + 36 * (size_t)i, out + 9 * (size_t)i);
}
extern "C" int h2_selftest_fe29_op(int field, int op, const int32_t in[36], int32_t out[9]) {
  if (!in || !out || op < 0 || op > 3) return H2_EINVAL;
  switch (field) {
    case 0: selftest_fe29_run<BN254_FQ>(op, in, out); return H2_OK;
    case 1: selftest_fe29_run<BN254_FR>(op, in, out); return H2_OK;
    case 2: selftest_fe29_run<PASTA_FP>(op, in, out); return H2_OK;
    case 3: selftest_fe29_run<PASTA_FQ>(op, in, out); return H2_OK;
  }
  return H2_EINVAL;
}
// n operand sets through the DEVICE instantiation, one kernel launch; host pointers in (36 limbs per set) and out (9)
extern "C" int h2_selftest_fe29_op_device(int field, int op, const int32_t* in, int32_t* out, size_t n) {
  std::lock_guard<std::recursive_mutex> lk(g_h2_mu);
  if (!g_h2.ready) return H2_ENOTINIT;
  if (!in || !out || n == 0 || n > (1u << 20) || field < 0 || field > 3 || op < 0 || op > 3) return H2_EINVAL;
  DevCtx& g_ctx = g_h2.ctx[0];
  DeviceGuard dg(g_ctx.device);
  const size_t in_bytes = n * 36 * 4, out_bytes = n * 9 * 4;
  ArenaLease stage(g_ctx.stage, in_bytes + out_bytes, g_ctx.stream);
  if (stage.rc != H2_OK) return stage.rc;
  int32_t* d_in = (int32_t*)g_ctx.stage.p;
  int32_t* d_out = (int32_t*)((char*)g_ctx.stage.p + in_bytes);
  H2_TRY(hipMemcpyAsync(d_in, in, in_bytes, hipMemcpyHostToDevice, g_ctx.stream));
  const dim3 grid((unsigned)((n + 63) / 64)), block(64);
  switch (field) {
    case 0: hipLaunchKernelGGL(selftest_fe29_kernel<BN254_FQ>, grid, block, 0, g_ctx.stream, op, d_in, d_out, (uint32_t)n); break;
    case 1: hipLaunchKernelGGL(selftest_fe29_kernel<BN254_FR>, grid, block, 0, g_ctx.stream, op, d_in, d_out, (uint32_t)n); break;
    case 2: hipLaunchKernelGGL(selftest_fe29_kernel<PASTA_FP>, grid, block, 0, g_ctx.stream, op, d_in, d_out, (uint32_t)n); break;
    default: hipLaunchKernelGGL(selftest_fe29_kernel<PASTA_FQ>, grid, block, 0, g_ctx.stream, op, d_in, d_out, (uint32_t)n); break;
  }
  if (int rc = launched(hipGetLastError(), "selftest_fe29_kernel"); rc != H2_OK) return rc;
  H2_TRY(hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, g_ctx.stream));
  return stage.wait();
}
// the same operand sets through BOTH forms of the product on the device: the compiler's (h2_field29.hpp) into out_cpp, the
// single-chain one (h2_field29_chain.hpp, as msm_chunk_kernel and the NTT pass instantiate it) into out_chain
template <class FP>
__global__ void __launch_bounds__(64) selftest_fe29_chain_kernel(int op, const int32_t* __restrict__ in, int32_t* __restrict__ out_cpp,
                                                                 int32_t* __restrict__ out_chain, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Fe29<FP> a[4];
  for (int k = 0; k < 4; k++)
    for (int l = 0; l < 9; l++) a[k].v[l] = in[36 * (size_t)i + 9 * k + l];
  Fe29<FP> r, c;
  switch (op) {
    case 0: r = fe29_mul(a[0], a[1]); c = Fe29Chain::mul(a[0], a[1]); break;
    case 1: r = fe29_sqr(a[0]); c = Fe29Chain::sqr(a[0]); break;
    case 2: r = fe29_mul_sub(a[0], a[1], a[2], a[3]); c = Fe29Chain::mul_sub(a[0], a[1], a[2], a[3]); break;
    default: r = fe29_mul_up(a[0], a[1]); c = Fe29Chain::mul_up(a[0], a[1]); break;
  }
  for (int l = 0; l < 9; l++) {
    out_cpp[9 * (size_t)i + l] = r.v[l];
    out_chain[9 * (size_t)i + l] = c.v[l];
  }
}
extern "C" int h2_selftest_fe29_chain_device(int field, int op, const int32_t* in, int32_t* out_cpp, int32_t* out_chain, size_t n) {
  std::lock_guard<std::recursive_mutex> lk(g_h2_mu);
  if (!g_h2.ready) return H2_ENOTINIT;
  // the chain forms exist for the Pasta fields only (p = 1 mod 2^29)
  if (!in || !out_cpp || !out_chain || n == 0 || n > (1u << 20) || field < 2 || field > 3 || op < 0 || op > 3) return H2_EINVAL;
  static_assert(chain29::covers<PASTA_FP>() && chain29::covers<PASTA_FQ>(), "the Pasta fields take the chain form");
  DevCtx& g_ctx = g_h2.ctx[0];
  DeviceGuard dg(g_ctx.device);
  const size_t in_bytes = n * 36 * 4, out_bytes = n * 9 * 4;
  ArenaLease stage(g_ctx.stage, in_bytes + 2 * out_bytes, g_ctx.stream);
  if (stage.rc != H2_OK) return stage.rc;
  int32_t* d_in = (int32_t*)g_ctx.stage.p;
  int32_t* d_cpp = (int32_t*)((char*)g_ctx.stage.p + in_bytes);
  int32_t* d_chain = (int32_t*)((char*)g_ctx.stage.p + in_bytes + out_bytes);
  H2_TRY(hipMemcpyAsync(d_in, in, in_bytes, hipMemcpyHostToDevice, g_ctx.stream));
  const dim3 grid((unsigned)((n + 63) / 64)), block(64);
  if (field == 2)
    hipLaunchKernelGGL(selftest_fe29_chain_kernel<PASTA_FP>, grid, block, 0, g_ctx.stream, op, d_in, d_cpp, d_chain, (uint32_t)n);
  else
    hipLaunchKernelGGL(selftest_fe29_chain_kernel<PASTA_FQ>, grid, block, 0, g_ctx.stream, op, d_in, d_cpp, d_chain, (uint32_t)n);
  if (int rc = launched(hipGetLastError(), "selftest_fe29_chain_kernel"); rc != H2_OK) return rc;
  H2_TRY(hipMemcpyAsync(out_cpp, d_cpp, out_bytes, hipMemcpyDeviceToHost, g_ctx.stream));
  H2_TRY(hipMemcpyAsync(out_chain, d_chain, out_bytes, hipMemcpyDeviceToHost, g_ctx.stream));
  return stage.wait();
}
extern "C" int h2_selftest_curve_op(int curve, int op, const uint64_t p[8], const uint64_t q[8], uint64_t out[8]) {
  const CurveOps* ops = ops_of(curve);
  if (!ops || !p || !q || !out) return H2_EINVAL;
  return ops->selftest_curve(op, p, q, out) == 0 ? H2_OK : H2_EINVAL;
}
// the working-form group law on raw operands, host instantiation: no GPU and no h2_init
extern "C" int h2_selftest_xyzz29_op(int curve, int op, const int32_t in[72], int32_t out[36]) {
  const CurveOps* ops = ops_of(curve);
  if (!ops || !in || !out || op < 0 || op > 3) return H2_EINVAL;
  return ops->selftest_xyzz29(op, in, out) == 0 ? H2_OK : H2_EINVAL;
}
// n operand pairs (72 limbs each, host pointer) through the DEVICE instantiation, one kernel launch, four lanes per pair;
// out: n x 4 x 36 limbs, a copy of the result from every lane of the quad
extern "C" int h2_selftest_xyzz29_op_device(int curve, int op, const int32_t* in, int32_t* out, size_t n) {
  std::lock_guard<std::recursive_mutex> lk(g_h2_mu);
  if (!g_h2.ready) return H2_ENOTINIT;
  const CurveOps* ops = ops_of(curve);
  if (!ops || !in || !out || n == 0 || n > (1u << 20) || op < 0 || op > 7) return H2_EINVAL;
  if (op >= 6 && !ops->base_chain29) return H2_EINVAL;       // the chain forms exist only for p = 1 mod 2^29
  DevCtx& g_ctx = g_h2.ctx[0];
  DeviceGuard dg(g_ctx.device);
  const size_t in_bytes = n * 72 * 4, out_bytes = n * 4 * 36 * 4;
  ArenaLease stage(g_ctx.stage, in_bytes + out_bytes, g_ctx.stream);
  if (stage.rc != H2_OK) return stage.rc;
  char* d = (char*)g_ctx.stage.p;
  H2_TRY(hipMemcpyAsync(d, in, in_bytes, hipMemcpyHostToDevice, g_ctx.stream));
  if (int rc = launched(ops->selftest_xyzz29_device(op, d, d + in_bytes, (uint32_t)n, g_ctx.stream), "selftest_xyzz29_kernel");
      rc != H2_OK)
    return rc;
  H2_TRY(hipMemcpyAsync(out, d + in_bytes, out_bytes, hipMemcpyDeviceToHost, g_ctx.stream));
  return stage.wait();
}
extern "C" int h2_selftest_digits(int curve, const uint64_t scalar[4], size_t n_for_geometry, uint32_t* out,
                                  uint32_t cap) {
  const CurveOps* ops = ops_of(curve);
  if (!ops || !scalar || !out) return H2_EINVAL;
  return ops->selftest_digits(scalar, n_for_geometry, out, cap);
}
// n element pairs through the DEVICE instantiation (one kernel launch); host pointers in and out
extern "C" int h2_selftest_curve_op_device(int curve, int op, const uint64_t* p, const uint64_t* q, uint64_t* out,
                                           size_t n) {
  std::lock_guard<std::recursive_mutex> lk(g_h2_mu);
  if (!g_h2.ready) return H2_ENOTINIT;
  const CurveOps* ops = ops_of(curve);
  if (!ops || !p || !q || !out || n == 0 || n > (1u << 20)) return H2_EINVAL;
  DevCtx& g_ctx = g_h2.ctx[0];
  DeviceGuard dg(g_ctx.device);
  ArenaLease stage(g_ctx.stage, 3 * n * 64, g_ctx.stream);
  if (stage.rc != H2_OK) return stage.rc;
  char* d = (char*)g_ctx.stage.p;
  H2_TRY(hipMemcpyAsync(d, p, n * 64, hipMemcpyHostToDevice, g_ctx.stream));
  H2_TRY(hipMemcpyAsync(d + n * 64, q, n * 64, hipMemcpyHostToDevice, g_ctx.stream));
  if (int rc = launched(ops->selftest_curve_device(op, d, d + n * 64, d + 2 * n * 64, (uint32_t)n, g_ctx.stream), "selftest_curve_kernel");
      rc != H2_OK)
    return rc;
  H2_TRY(hipMemcpyAsync(out, d + 2 * n * 64, n * 64, hipMemcpyDeviceToHost, g_ctx.stream));
  return stage.wait();
}

extern "C" int h2_selftest_field_op_device(int field, int op, const uint64_t* a, const uint64_t* b, uint64_t* out,
                                           size_t n) {
  std::lock_guard<std::recursive_mutex> lk(g_h2_mu);
  if (!g_h2.ready) return H2_ENOTINIT;
  if (!a || !b || !out || n == 0 || n > (1u << 24) || field < 0 || field > 3) return H2_EINVAL;
  const CurveOps* ops = field < 2 ? curve_ops_bn254() : curve_ops_pallas();
  const int which = field & 1;
  DevCtx& g_ctx = g_h2.ctx[0];
  DeviceGuard dg(g_ctx.device);
  ArenaLease stage(g_ctx.stage, 3 * n * 32, g_ctx.stream);
  if (stage.rc != H2_OK) return stage.rc;
  char* d = (char*)g_ctx.stage.p;
  H2_TRY(hipMemcpyAsync(d, a, n * 32, hipMemcpyHostToDevice, g_ctx.stream));
  H2_TRY(hipMemcpyAsync(d + n * 32, b, n * 32, hipMemcpyHostToDevice, g_ctx.stream));
  if (int rc = launched(ops->selftest_field_device(which, op, d, d + n * 32, d + 2 * n * 32, (uint32_t)n, g_ctx.stream), "selftest_field_kernel");
      rc != H2_OK)
    return rc;
  H2_TRY(hipMemcpyAsync(out, d + 2 * n * 32, n * 32, hipMemcpyDeviceToHost, g_ctx.stream));
  return stage.wait();
}

// test hooks around the MSM workspace (include/h2hip_selftest.h)
extern "C" int h2_selftest_msm_guard(int on) {
  std::lock_guard<std::recursive_mutex> lk(g_h2_mu);
  g_knobs.msm_guard = on != 0;
  g_knobs.msm_guard_poke = on == 2;
  g_knobs.sort2_pack = on != 3;          // guard(3): the unpacked forms -- the two-level sort keeps the low key bits in the
                                         // side array, the staged scatter a reference and a 16-bit bucket per entry
  g_counts.guard_launches = g_counts.guard_violations = 0;
  g_counts.guard_first.clear();
  return H2_OK;
}
extern "C" int h2_selftest_msm_guard_report(uint64_t out[2], char* first, size_t cap) {
  std::lock_guard<std::recursive_mutex> lk(g_h2_mu);
  if (!out) return H2_EINVAL;
  out[0] = g_counts.guard_launches;
  out[1] = g_counts.guard_violations;
  if (first && cap) {
    snprintf(first, cap, "%s", g_counts.guard_first.c_str());
  }
  return H2_OK;
}
// host only: msm_device_run's plan (msm_plan_group) of an (n_bases, n, m, col_stride) launch: the workspace and the bounds
// proof on it; out[0..7] = window bits, windows, buckets, tile, staged, two-level sort, entries per thread, regions.
// Returns H2_OK, or H2_EINVAL with the violated condition in h2_last_device_error().
extern "C" int h2_selftest_msm_check(int curve, size_t n_bases, size_t n, size_t m, size_t col_stride, int guard, uint64_t out[8]) {
  std::lock_guard<std::recursive_mutex> lk(g_h2_mu);
  const CurveOps* ops = ops_of(curve);
  if (!ops || n == 0 || m == 0 || n > n_bases) return H2_EINVAL;
  const MsmGeom g = msm_geometry(n_bases, ops->scalar_bits);
  // a batch wider than one launch takes runs in column groups; the first (widest) group is checked
  const MsmGroupPlan plan = msm_plan_group(g, n_bases, n, m, col_stride, guard != 0, true);
  if (plan.cols == 0) return H2_EINVAL;
  if (m > plan.cols && col_stride < n) { g_h2.last_error = "msm launch geometry: col_stride >= n"; return H2_EINVAL; }
  const MsmWorkspace& ws = plan.ws;
  if (out) {
    out[0] = g.c; out[1] = g.W; out[2] = g.B; out[3] = ws.sort2 ? ws.s2.tile : ws.tile;
    out[4] = ws.staged; out[5] = ws.sort2; out[6] = ws.T; out[7] = ws.n_regions;
  }
  if (plan.broken) {
    g_h2.last_error = std::string("msm launch geometry: ") + plan.broken;
    return H2_EINVAL;
  }
  return H2_OK;
}
// host only: the layout and the bounds proof of a table-free launch (h2_msm_points*) of m columns of n scalars, as
// msm_points_plan_group gives them to msm_points_run; out: include/h2hip_selftest.h
extern "C" int h2_selftest_msm_points_check(int curve, size_t n, size_t m, size_t col_stride, int guard, uint64_t out[8]) {
  std::lock_guard<std::recursive_mutex> lk(g_h2_mu);
  if (!curve_ok(curve) || !out || n == 0 || m == 0 || n > MSM_POINTS_MAX_N) return H2_EINVAL;
  if (col_stride < n) { g_h2.last_error = "msm points launch geometry: col_stride >= n"; return H2_EINVAL; }
  const MsmGeom g = msm_points_geometry(n, ops_of(curve)->scalar_bits);
  // a batch wider than one launch runs in column groups; the first (widest) group is checked
  const MsmGroupPlan plan = msm_points_plan_group(g, n, m, col_stride, guard != 0);
  if (plan.cols == 0) return H2_EINVAL;
  const MsmWorkspace& ws = plan.ws;
  out[0] = g.c; out[1] = g.W; out[2] = g.B; out[3] = ws.tile; out[4] = (uint64_t)g.W * g.B * 4; out[5] = plan.cols;
  out[6] = ws.T; out[7] = ws.n_regions;
  if (plan.broken) {
    g_h2.last_error = std::string("msm points launch geometry: ") + plan.broken;
    return H2_EDEVICE;
  }
  return H2_OK;
}
extern "C" int h2_selftest_set_msm_points_small_max(size_t n) {
  std::lock_guard<std::recursive_mutex> lk(g_h2_mu);
  g_knobs.points_small_max = n == SIZE_MAX ? MSM_POINTS_SMALL_MAX : n;
  return H2_OK;
}
// lanes per butterfly of the group FFT's stage kernel (h2_group_fft.hpp): 1 or 4 forces that form, 0 restores by size
extern "C" int h2_selftest_set_gfft_lanes(int lanes) {
  std::lock_guard<std::recursive_mutex> lk(g_h2_mu);
  if (lanes != 0 && lanes != 1 && lanes != 4) return H2_EINVAL;
  g_knobs.gfft_lanes = lanes;
  return H2_OK;
}
// host only: glv_split of `curve`'s scalar field on a canonical k; out = |k1| then |k2|, five words each, bit 31 of the
// fifth word the sign
extern "C" int h2_selftest_glv_split(int curve, const uint64_t k[4], uint32_t out[10]) {
  const CurveOps* ops = ops_of(curve);
  if (!ops || !k || !out) return H2_EINVAL;
  ops->selftest_glv_split(k, out);
  return H2_OK;
}
extern "C" int h2_selftest_glv_constants(int curve, uint64_t lambda[4], uint64_t beta[4], uint32_t* glv_bits) {
  const CurveOps* ops = ops_of(curve);
  if (!ops || !lambda || !beta || !glv_bits) return H2_EINVAL;
  ops->selftest_glv_constants(lambda, beta);
  *glv_bits = (uint32_t)ops->glv_bits;
  return H2_OK;
}
// host only: the sort front of a launch of m columns of n scalars against n_bases bases, as msm_plan_group lays it out
// for msm_device_run (`pack` = 0: with the unpacked forms, as under h2_selftest_msm_guard(3)); out: include/h2hip_selftest.h
extern "C" int h2_selftest_msm_front(int curve, size_t n_bases, size_t n, size_t m, int pack, uint64_t out[12]) {
  std::lock_guard<std::recursive_mutex> lk(g_h2_mu);
  const CurveOps* ops = ops_of(curve);
  if (!ops || !out || n == 0 || m == 0 || n > n_bases || n_bases >= (1ull << 31)) return H2_EINVAL;
  const MsmGeom g = msm_geometry(n_bases, ops->scalar_bits);
  const MsmGroupPlan plan = msm_plan_group(g, n_bases, n, m, n, false, pack != 0);
  if (plan.cols < m) return H2_EINVAL;        // one launch only
  const MsmWorkspace& ws = plan.ws;
  const char* broken = plan.broken;
  if (broken) g_h2.last_error = std::string("msm launch geometry: ") + broken;
  out[0] = ws.sort2 ? ws.s2.tile : ws.tile; out[1] = ws.staged; out[2] = ws.stage_lds; out[3] = ws.pack.on;
  out[4] = ws.pack.bbits; out[5] = ws.pack.ibits; out[6] = ws.pack.wbits; out[7] = broken ? 0 : 1;
  out[8] = msm_effective_t((uint32_t)ws.E, ws.T); out[9] = MSM_HOT_SPAN; out[10] = MSM_HOT_SEG; out[11] = ws.max_tasks;
  return H2_OK;
}
// host only: the fix-up kernel's share of the same layout -- of the first launch, where msm_plan_group cuts the m
// columns into several; out: include/h2hip_selftest.h
extern "C" int h2_selftest_msm_fixup(int curve, size_t n_bases, size_t n, size_t m, uint64_t out[4]) {
  std::lock_guard<std::recursive_mutex> lk(g_h2_mu);
  const CurveOps* ops = ops_of(curve);
  if (!ops || !out || n == 0 || m == 0 || n > n_bases || n_bases >= (1ull << 31)) return H2_EINVAL;
  const MsmGeom g = msm_geometry(n_bases, ops->scalar_bits);
  const MsmGroupPlan plan = msm_plan_group(g, n_bases, n, m, n, false, true);
  const MsmWorkspace& ws = plan.ws;
  if (plan.broken) {
    g_h2.last_error = std::string("msm launch geometry: ") + plan.broken;
    return H2_EINVAL;
  }
  out[0] = ws.log_f; out[1] = ws.K << ws.log_f; out[2] = ws.pieces; out[3] = ws.T;
  return H2_OK;
}
// scratch arenas of the current context: out = {allocations (first use or growth), cross-stream hand-overs (event waits),
// MSM slots taken over, NTT slots taken over}
extern "C" int h2_selftest_arena_stats(uint64_t out[4]) {
  std::lock_guard<std::recursive_mutex> lk(g_h2_mu);
  DevCtx* c = g_h2.ready ? ctx_current() : nullptr;
  if (!c || !out) return H2_EINVAL;
  out[0] = g_counts.arena_growths;
  out[1] = g_counts.arena_waits;
  out[2] = c->msm_ws.takeovers;
  out[3] = c->ntt_ws.takeovers;
  return H2_OK;
}
// host only: the sort's block -> (column, tile) mapping for `tiles` tiles per column and m columns: every block of
// the grid is either dead or maps to a (column < m, tile < tiles) pair that no other block takes, and all pairs are taken
extern "C" int h2_selftest_msm_tiles(uint32_t tiles, uint32_t m) {
  if (tiles == 0 || m == 0 || (uint64_t)tiles * m > (1u << 24)) return H2_EINVAL;
  const uint32_t grid = msm_tile_grid(tiles, m);
  std::vector<uint8_t> seen((size_t)tiles * m, 0);
  size_t live = 0;
  for (uint32_t b = 0; b < grid; b++) {
    const MsmTileId t = msm_tile_id_of(b, tiles, m);
    if (!t.live) continue;
    if (t.col >= m || t.tile >= tiles || t.group >= MSM_XCDS || seen[(size_t)t.col * tiles + t.tile]) return H2_EINVAL;
    seen[(size_t)t.col * tiles + t.tile] = 1;
    live++;
  }
  return live == (size_t)tiles * m ? H2_OK : H2_EINVAL;
}

// test hook: lower the sort's entry limit so that the grouped-columns path is reached at small sizes (0 = default)
extern "C" int h2_selftest_set_msm_max_entries(uint64_t limit) {
  std::lock_guard<std::recursive_mutex> lk(g_h2_mu);
  g_knobs.msm_max_entries = (limit > 0 && limit < (1ull << 31) - 1) ? limit : (1ull << 31) - 1;
  return H2_OK;
}

// measured integer ceiling: dependent 9 x 29-bit Montgomery products of `curve`'s base field at `waves_per_simd`
// resident waves per SIMD on every CU of the current device
extern "C" int h2_selftest_modmul_rate(int curve, int waves_per_simd, int iters, double* modmul_per_s) {
  std::lock_guard<std::recursive_mutex> lk(g_h2_mu);
  if (!g_h2.ready) return H2_ENOTINIT;
  const CurveOps* ops = ops_of(curve);
  if (!ops || !modmul_per_s || waves_per_simd < 1 || waves_per_simd > 8 || iters < 1 || iters > (1 << 20)) return H2_EINVAL;
  DevCtx* c = ctx_current();
  if (!c) return H2_EINVAL;
  hipDeviceProp_t prop;
  H2_TRY(hipGetDeviceProperties(&prop, c->device));
  return launched(ops->modmul_rate(prop.multiProcessorCount * waves_per_simd, iters, c->stream, modmul_per_s), "modmul_rate_kernel");
}

// ---- the IPA prover's transcript step (h2_ipa_prove.hpp): the host instantiation of what a lane of the kernel runs -----
namespace {
template <class FP>
void ipa_inv_run(int form, const uint64_t a[4], uint64_t out[4]) {
  Fe<FP> x;
  memcpy(x.v, a, 32);
  const Fe<FP> r = form ? fe_inv(x) : fe_inv_divsteps(x);
  memcpy(out, r.v, 32);
}
template <class CV>
void ipa_step_run(int form, const uint8_t* state_in, const uint64_t* lr, const uint64_t* lrf, uint8_t* wire, uint8_t* state_out,
                  uint64_t* out, uint32_t* status) {
  using FS = typename CV::Scalar;
  uint32_t ring[64] = {}, st[TRANSCRIPT_STATE_BYTES / 4], w[16];
  memcpy(st, state_in, TRANSCRIPT_STATE_BYTES);
  B2bLane<1> b;
  b.load(st, ring);
  Fe<typename CV::Base> pts[4];
  for (int i = 0; i < 4; i++) memcpy(pts[i].v, lr + 4 * i, 32);
  const Fe<FS> u = ipa_step_points<CV, 1>(b, pts, w);
  Fe<FS> l, r, f, uinv;
  memcpy(l.v, lrf, 32);
  memcpy(r.v, lrf + 4, 32);
  memcpy(f.v, lrf + 8, 32);
  *status = form ? ipa_step_fold<FS, 1>(u, l, r, f, uinv) : ipa_step_fold<FS, 0>(u, l, r, f, uinv);
  b.store(st);
  memcpy(wire, w, 64);
  memcpy(state_out, st, TRANSCRIPT_STATE_BYTES);
  memcpy(out, u.v, 32);
  memcpy(out + 4, uinv.v, 32);
  memcpy(out + 8, f.v, 32);
}
template <class FS>
void ipa_fold_run(int form, const uint64_t* in, uint64_t* out, uint32_t* status) {
  Fe<FS> u, l, r, f, uinv;
  memcpy(u.v, in, 32);
  memcpy(l.v, in + 4, 32);
  memcpy(r.v, in + 8, 32);
  memcpy(f.v, in + 12, 32);
  *status = form ? ipa_step_fold<FS, 1>(u, l, r, f, uinv) : ipa_step_fold<FS, 0>(u, l, r, f, uinv);
  memcpy(out, uinv.v, 32);
  memcpy(out + 4, f.v, 32);
}
template <class FS>
void ipa_scalar_run(const uint8_t* state_in, const uint64_t* s, uint8_t* canon, uint8_t* state_out) {
  uint32_t ring[64] = {}, st[TRANSCRIPT_STATE_BYTES / 4], w[8];
  memcpy(st, state_in, TRANSCRIPT_STATE_BYTES);
  B2bLane<1> b;
  b.load(st, ring);
  Fe<FS> x;
  memcpy(x.v, s, 32);
  ipa_step_scalar<FS, 1>(b, x, w);
  b.store(st);
  memcpy(canon, w, 32);
  memcpy(state_out, st, TRANSCRIPT_STATE_BYTES);
}
}  // namespace
extern "C" int h2_selftest_field_inv(int field, int form, const uint64_t a[4], uint64_t out[4]) {
  if (!a || !out || form < 0 || form > 1) return H2_EINVAL;
  switch (field) {
    case 0: ipa_inv_run<BN254_FQ>(form, a, out); return H2_OK;
    case 1: ipa_inv_run<BN254_FR>(form, a, out); return H2_OK;
    case 2: ipa_inv_run<PASTA_FP>(form, a, out); return H2_OK;
    case 3: ipa_inv_run<PASTA_FQ>(form, a, out); return H2_OK;
  }
  return H2_EINVAL;
}
extern "C" int h2_selftest_ipa_step(int curve, int form, const uint8_t state_in[208], const uint64_t lr[16], const uint64_t lrf[12],
                                    uint8_t wire[64], uint8_t state_out[208], uint64_t out[12], uint32_t* status) {
  if (!state_in || !lr || !lrf || !wire || !state_out || !out || !status || form < 0 || form > 1) return H2_EINVAL;
  if (curve == H2_PALLAS)
    ipa_step_run<PALLAS_CURVE>(form, state_in, lr, lrf, wire, state_out, out, status);
  else if (curve == H2_VESTA)
    ipa_step_run<VESTA_CURVE>(form, state_in, lr, lrf, wire, state_out, out, status);
  else
    return H2_EINVAL;
  return H2_OK;
}
extern "C" int h2_selftest_ipa_fold(int curve, int form, const uint64_t in[16], uint64_t out[8], uint32_t* status) {
  if (!in || !out || !status || form < 0 || form > 1) return H2_EINVAL;
  if (curve == H2_PALLAS)
    ipa_fold_run<PALLAS_CURVE::Scalar>(form, in, out, status);
  else if (curve == H2_VESTA)
    ipa_fold_run<VESTA_CURVE::Scalar>(form, in, out, status);
  else
    return H2_EINVAL;
  return H2_OK;
}
extern "C" int h2_selftest_ipa_step_scalar(int curve, const uint8_t state_in[208], const uint64_t s[4], uint8_t canon[32],
                                           uint8_t state_out[208]) {
  if (!state_in || !s || !canon || !state_out) return H2_EINVAL;
  if (curve == H2_PALLAS)
    ipa_scalar_run<PALLAS_CURVE::Scalar>(state_in, s, canon, state_out);
  else if (curve == H2_VESTA)
    ipa_scalar_run<VESTA_CURVE::Scalar>(state_in, s, canon, state_out);
  else
    return H2_EINVAL;
  return H2_OK;
}
// tests and tools only: the inversion of the step kernel (0: divsteps, the product's; 1: fe_inv's Fermat chain)
extern "C" int h2_selftest_set_ipa_inv_form(int form) {
  std::lock_guard<std::recursive_mutex> lk(g_h2_mu);
  if (form < 0 || form > 1) return H2_EINVAL;
  g_knobs.ipa_inv_form = form;
  return H2_OK;
}

// ---- Poseidon (h2_poseidon.hpp) --------------------------------------------------------------------------------------
namespace {
// host only: the kernels' permutation and sponge templates instantiated on the host, on `elems` table entries as Montgomery
// limbs
int poseidon_selftest_run(int curve, uint32_t width, uint32_t r_f, uint32_t r_p, int form, int op, uint32_t len,
                          const std::vector<uint64_t>& api, size_t elems, const uint64_t* in, uint64_t* out) {
  const PoseidonOps* ops = poseidon_ops_of(curve);
  std::vector<int32_t> table(9 * elems);
  ops->table(api.data(), elems, table.data());
  uint64_t cap[4];
  poseidon_capacity_mont(curve, len, cap);
  return ops->selftest(width, form, op, len, r_f, r_p, table.data(), cap, in, out) == 0 ? H2_OK : H2_EINVAL;
}
}  // namespace
// width 3, on the table h2_poseidon_constants' values make: op 0 permutes one state, op 1 is ConstantLength<2> of two elements
extern "C" int h2_selftest_poseidon(int curve, uint32_t r_f, uint32_t r_p, int op, const uint64_t* in, uint64_t* out) {
  if (!curve_ok(curve) || !in || !out || op < 0 || op > 1) return H2_EINVAL;
  size_t elems = 0;
  if (h2_poseidon_constants((h2_curve_t)curve, r_f, r_p, nullptr, 0, &elems) != H2_EINVAL || elems == 0) return H2_EINVAL;
  std::vector<uint64_t> api(4 * elems);
  if (int rc = h2_poseidon_constants((h2_curve_t)curve, r_f, r_p, api.data(), elems, &elems); rc != H2_OK) return rc;
  return poseidon_selftest_run(curve, 3, r_f, r_p, 0, op, 2, api, elems, in, out);
}
// the widths 5 and 9: the table as the kernels read it (before the change to the working form)
extern "C" int h2_selftest_poseidon_wide_table(int curve, uint32_t width, uint32_t r_f, uint32_t r_p, uint64_t* out, size_t cap_elems,
                                               size_t* n_elems) {
  size_t dense = 0;
  if (!n_elems || (width != 5 && width != 9) ||
      h2_poseidon_wide_constants((h2_curve_t)curve, width, r_f, r_p, nullptr, 0, &dense) != H2_EINVAL || dense == 0)
    return H2_EINVAL;
  const size_t need = poseidon_table_elems(width, r_f, r_p);
  *n_elems = need;
  if (!out || cap_elems < need) return H2_EINVAL;
  return poseidon_wide_table_mont(curve, width, r_f, r_p, true, out) ? H2_OK : H2_EINVAL;
}
extern "C" int h2_selftest_poseidon_wide(int curve, uint32_t width, uint32_t r_f, uint32_t r_p, int form, int op, uint32_t len,
                                         const uint64_t* in, uint64_t* out) {
  if (!curve_ok(curve) || !in || !out || op < 0 || op > 1 || (op == 1 && (len == 0 || len > 65535))) return H2_EINVAL;
  size_t elems = 0;
  if (h2_selftest_poseidon_wide_table(curve, width, r_f, r_p, nullptr, 0, &elems) != H2_EINVAL || elems == 0) return H2_EINVAL;
  std::vector<uint64_t> api(4 * elems);
  if (int rc = h2_selftest_poseidon_wide_table(curve, width, r_f, r_p, api.data(), elems, &elems); rc != H2_OK) return rc;
  return poseidon_selftest_run(curve, width, r_f, r_p, form, op, len, api, elems, in, out);
}
// tests and tools only: the partial rounds of h2_poseidon_wide_permute_device's kernel (0: the width's own form, 1: dense, 2: sparse)
extern "C" int h2_selftest_set_poseidon_wide_form(int form) {
  std::lock_guard<std::recursive_mutex> lk(g_h2_mu);
  if (form < 0 || form > 2) return H2_EINVAL;
  g_knobs.poseidon_wide_form = form;
  return H2_OK;
}
// tests and tools only: the widest Merkle level the tail launch takes (a power of two up to POSEIDON_MERKLE_TAIL_MAX; 0
// restores the default), and the product form of the hash kernel (0: by size, 1: the compiler's, 2: single-chain where the
// field has it)
extern "C" int h2_selftest_set_poseidon_merkle_tail(uint32_t nodes) {
  std::lock_guard<std::recursive_mutex> lk(g_h2_mu);
  if (nodes > POSEIDON_MERKLE_TAIL_MAX || (nodes & (nodes - 1))) return H2_EINVAL;
  g_knobs.poseidon_merkle_tail = nodes;
  return H2_OK;
}
extern "C" int h2_selftest_set_poseidon_form(int form) {
  std::lock_guard<std::recursive_mutex> lk(g_h2_mu);
  if (form < 0 || form > 2) return H2_EINVAL;
  g_knobs.poseidon_form = form;
  return H2_OK;
}
// tests and tools only: the form of h2_poseidon_merkle_verify_device's walker and of h2_poseidon_merkle_update_device's level
// and top launches (0: by size, 1: one lane per hash, 2: four lanes per hash)
extern "C" int h2_selftest_set_poseidon_walk_form(int form) {
  std::lock_guard<std::recursive_mutex> lk(g_h2_mu);
  if (form < 0 || form > 2) return H2_EINVAL;
  g_knobs.poseidon_walk_form = form;
  return H2_OK;
}
