// h2_capi.hip -- implementation of include/h2hip.h (the drop-in C ABI).
//
// One context per process, bound to one GPU.  Every entry point validates its arguments,
// takes the context mutex, enqueues on the context stream (or the caller's) and reports
// errors as h2_status_t values: nothing throws or aborts across the ABI
// (the reference's panics -- /root/reference/circuits/src/utils.rs:91,120 `.expect(..)`,
// best_multiexp's assert_eq!(coeffs.len(), bases.len()) -- become H2_EINVAL here).
#include "h2_internal.hpp"

#include <sys/random.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <functional>
#include <optional>

#include "h2_expr_program.hpp"
#include "h2_host.hpp"
#include "h2_ipa.hpp"
#include "h2_ipa_verify.hpp"
#include "h2_ipa_prove.hpp"
#include "h2_lookup.hpp"
#include "h2_ntt.hpp"
#include "h2_permutation.hpp"
#include "h2_poly.hpp"
#include "h2_poseidon.hpp"
#include "h2_poseidon_host.hpp"

using namespace h2;

namespace h2 {

Global g_h2;
std::recursive_mutex g_h2_mu;
TestKnobs g_knobs;
TestCounters g_counts;

int dev_fail(hipError_t e, const char* where) {
  char buf[256];
  snprintf(buf, sizeof buf, "%s: %s", where, hipGetErrorString(e));
  g_h2.last_error = buf;
  return H2_EDEVICE;
}

bool curve_ok(int c) { return c == H2_BN254 || c == H2_PALLAS || c == H2_VESTA; }

const CurveOps* ops_of(int curve) {
  switch (curve) {
    case H2_BN254: return curve_ops_bn254();
    case H2_PALLAS: return curve_ops_pallas();
    case H2_VESTA: return curve_ops_vesta();
  }
  return nullptr;
}
const PoseidonOps* poseidon_ops_of(int curve) {
  return curve == H2_BN254 ? poseidon_ops_bn254() : curve == H2_PALLAS ? poseidon_ops_pallas() : poseidon_ops_vesta();
}

DevCtx* ctx_current() {
  if (!g_h2.ready || g_h2.ctx.empty()) return nullptr;
  if (g_h2.ctx.size() == 1) return &g_h2.ctx[0];
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess) return nullptr;
  for (auto& c : g_h2.ctx)
    if (c.device == dev) return &c;
  return nullptr;
}
size_t ctx_index(const DevCtx* c) { return (size_t)(c - &g_h2.ctx[0]); }

int device_alloc(void** p, size_t bytes, const char* what) {
  hipError_t e = hipMalloc(p, bytes);
  if (e == hipSuccess) return H2_OK;
  (void)hipGetLastError();
  *p = nullptr;
  g_h2.last_error = std::string("hipMalloc(") + what + "): " + hipGetErrorString(e);
  return H2_ENOMEM;
}

// ---- arenas ----------------------------------------------------------------------------------
ArenaLease::ArenaLease(Arena& arena, size_t want, hipStream_t stream) : a(arena), s(stream) { rc = acquire(want); }
int ArenaLease::acquire(size_t want) {
  clean_bytes = a.bytes < want ? 0 : a.clean_bytes;   // this user takes over the region and may overwrite it
  a.clean_bytes = 0;
  if (a.bytes < want) {
    g_counts.arena_growths++;
    if (a.p) {
      // rare: a larger call than any before.  Work enqueued on other streams may still use the arena.
      H2_TRY(hipDeviceSynchronize());
      (void)hipFree(a.p);
      a.p = nullptr;
      a.bytes = 0;
      a.used = false;
    }
    const size_t sz = want + (want >> 3);  // head-room so slightly larger calls do not reallocate
    if (int st = device_alloc(&a.p, sz, "arena"); st != H2_OK) return st;
    a.bytes = sz;
  }
  if (!a.ev) H2_TRY(hipEventCreateWithFlags(&a.ev, hipEventDisableTiming));
  if (a.used && a.last != s) {                                         // order behind the previous user
    g_counts.arena_waits++;
    H2_TRY(hipStreamWaitEvent(s, a.ev, 0));
  }
  return H2_OK;
}
int ArenaLease::release() {
  released = true;
  H2_TRY(hipEventRecord(a.ev, s));
  a.last = s;
  a.used = true;
  return H2_OK;
}
int ArenaLease::wait() {
  H2_TRY(hipStreamSynchronize(s));
  released = true;   // the arena is idle: no event has to order a later user behind this use
  return H2_OK;
}
ArenaLease::~ArenaLease() noexcept {
  if (rc != H2_OK || released) return;
  if (hipEventRecord(a.ev, s) == hipSuccess) {
    a.last = s;
    a.used = true;
  } else {
    (void)hipGetLastError();
  }
}
static void arena_free(Arena& a) {
  if (a.p) (void)hipFree(a.p);
  if (a.ev) (void)hipEventDestroy(a.ev);
  a = Arena{};
}

// ---- bases ---------------------------------------------------------------------------------
// d_affine lives on context `src`; the table is built there and copied to every other context
static int register_device(DevCtx& src, int curve, const void* d_affine, size_t n, uint64_t* handle_out) {
  if (!curve_ok(curve) || !d_affine || !handle_out || n == 0) return H2_EINVAL;
  const CurveOps* ops = ops_of(curve);
  MsmGeom g = msm_geometry(n, ops->scalar_bits);
  if ((uint64_t)g.W * n >= (1ull << 31)) return H2_EINVAL;
  BasesEntry be{};
  be.curve = curve;
  be.n = n;
  be.geom = g;
  be.table_bytes = (size_t)g.W * n * 64;
  be.table.assign(g_h2.ctx.size(), nullptr);
  auto fail = [&](int rc) {
    for (size_t i = 0; i < be.table.size(); i++)
      if (be.table[i]) {
        DeviceGuard dg(g_h2.ctx[i].device);
        (void)hipFree(be.table[i]);
      }
    return rc;
  };
  for (size_t i = 0; i < g_h2.ctx.size(); i++) {
    DeviceGuard dg(g_h2.ctx[i].device);
    if (int rc = device_alloc(&be.table[i], be.table_bytes, "table"); rc != H2_OK) return fail(rc);
  }
  const size_t si = ctx_index(&src);
  {
    DeviceGuard dg(src.device);
    // the points are checked while the table is built: a counter in the (otherwise idle) scan arena
    ArenaLease scan_ws(src.div_ws, sizeof(uint32_t), src.stream);
    if (scan_ws.rc != H2_OK) return fail(scan_ws.rc);
    uint32_t* d_bad = (uint32_t*)scan_ws.a.p;
    uint32_t bad = 0;
    // the table kernel's scratch (80 bytes per table entry) is the MSM workspace, idle while bases are being registered
    ArenaLease table_ws(src.msm_ws.of(src.stream), be.table_bytes / 64 * MSM_TABLE_SCRATCH, src.stream);
    if (table_ws.rc != H2_OK) return fail(table_ws.rc);
    hipError_t e = hipMemsetAsync(d_bad, 0, 4, src.stream);
    if (e == hipSuccess) e = ops->table_build(d_affine, be.table[si], table_ws.a.p, (uint32_t)n, g, d_bad, src.stream);
    if (e == hipSuccess) e = hipMemcpyAsync(&bad, d_bad, 4, hipMemcpyDeviceToHost, src.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(src.stream);
    if (e != hipSuccess) return fail(dev_fail(e, "msm_table_kernel"));
    (void)scan_ws.release();
    (void)table_ws.release();
    if (bad) {
      g_h2.last_error = "bases: " + std::to_string(bad) + " point(s) not on the curve";
      return fail(H2_EINVAL);
    }
    for (size_t i = 0; i < g_h2.ctx.size(); i++) {
      if (i == si) continue;
      e = hipMemcpyPeer(be.table[i], g_h2.ctx[i].device, be.table[si], src.device, be.table_bytes);
      if (e != hipSuccess) return fail(dev_fail(e, "hipMemcpyPeer(table)"));
    }
  }
  uint64_t h = g_h2.next_handle++;
  g_h2.bases[h] = be;
  *handle_out = h;
  return H2_OK;
}

// ---- MSM -----------------------------------------------------------------------------------
int msm_common_checks(int curve, uint64_t handle, size_t first, size_t n, size_t m, const BasesEntry** be) {
  if (!g_h2.ready) return H2_ENOTINIT;
  if (!curve_ok(curve) || m == 0) return H2_EINVAL;
  auto it = g_h2.bases.find(handle);
  if (it == g_h2.bases.end()) return H2_EHANDLE;
  if (it->second.curve != curve) return H2_EINVAL;
  if (first > it->second.n || n > it->second.n - first) return H2_EINVAL;  // best_multiexp: assert_eq!(coeffs.len(), bases.len())
  *be = &it->second;
  return H2_OK;
}

// Columns per launch: the sort indexes its m * W * n entries with 32 bits, so a wide batch of long columns
// (2^24 rows x 8 columns) goes through in groups of columns, one after the other on the same stream and workspace.
size_t msm_cols_per_launch(const MsmGeom& geom, size_t n) {
  const uint64_t per_col = (uint64_t)geom.W * n;
  const uint64_t by_entries = g_knobs.msm_max_entries / per_col;
  uint64_t by_keys = ((1ull << 31) - 1) / geom.B;
  // wide windows go through the two-level sort, whose one-block scan of the coarse bins holds S2_MAX_H of them: rather
  // than fall back to the one-level sort's scattered stores (which windows beyond 16 bits cannot use at all), a wider
  // batch runs in groups of that many columns
  if (geom.B > 4096) {
    const uint64_t by_bins = S2_MAX_H / msm_sort2_geom(n, geom).Hc;
    if (by_bins >= 1 && by_bins < by_keys) by_keys = by_bins;
  }
  return (size_t)(by_entries < by_keys ? by_entries : by_keys);   // 0: a single column is already too long
}

// guard mode (tests only, h2_selftest_msm_guard): count the red-zone bytes that the launch sequence just enqueued changed
// (synchronous) and note the first overrun; `m` (the caller's columns) and `what` describe the launch in that note
static int msm_guard_inspect(const MsmWorkspace& ws, char* ws_base, hipStream_t stream, size_t m, const char* what) {
  void* d_bad = nullptr;
  if (int rc = device_alloc(&d_bad, ws.n_regions * 4, "guard"); rc != H2_OK) return rc;
  DeviceBuffer owner(d_bad);
  std::vector<uint32_t> bad(ws.n_regions, 0);
  H2_TRY(hipMemsetAsync(d_bad, 0, ws.n_regions * 4, stream));
  if (g_knobs.msm_guard_poke)        // the checker's own test: one byte just behind the second region
    H2_TRY(hipMemsetAsync(ws_base + ws.regions[1].off + ws.regions[1].bytes, 0, 1, stream));
  hipLaunchKernelGGL(msm_guard_check_kernel, dim3(ws.n_regions), dim3(256), 0, stream, (const uint8_t*)ws_base, ws, (uint32_t*)d_bad);
  H2_TRY(hipMemcpyAsync(bad.data(), d_bad, ws.n_regions * 4, hipMemcpyDeviceToHost, stream));
  H2_TRY(hipStreamSynchronize(stream));
  g_counts.guard_launches++;
  for (uint32_t r = 0; r < ws.n_regions; r++)
    if (bad[r]) {
      if (!g_counts.guard_violations)
        g_counts.guard_first = std::string(ws.regions[r].name) + ": " + std::to_string(bad[r]) + " byte(s) behind the region, n=" +
                               std::to_string(ws.n) + " m=" + std::to_string(m) + what;
      g_counts.guard_violations++;
    }
  return H2_OK;
}

// One planned launch sequence on the MSM workspace of `stream`, leased from its first kernel to its last:
// launch(ws_base, zeroed) -> hipError_t enqueues it (`label` names it in an error), then finish(ws_base) -> status what
// still reads the workspace.  A plan whose bounds proof failed ("<route> launch geometry: ...") enqueues nothing.
template <class Launch, class Finish>
static int msm_run_group(DevCtx& c, hipStream_t stream, const MsmGroupPlan& plan, const char* route, const char* label, size_t m,
                         const char* guard_what, Launch&& launch, Finish&& finish) {
  const MsmWorkspace& ws = plan.ws;
  ArenaLease lease(c.msm_ws.of(stream), ws.total, stream);
  if (lease.rc != H2_OK) return lease.rc;
  Arena& A = lease.a;
  // the plan proved the layout against its own size; the arena the lease handed out must hold it
  if (const char* broken = plan.broken ? plan.broken : ws.total <= A.bytes ? nullptr : "ws.total <= arena_bytes") {
    g_h2.last_error = std::string(route) + " launch geometry: " + broken;
    return H2_EDEVICE;
  }
  const bool guard = g_knobs.msm_guard;
  if (guard) H2_TRY(hipMemsetAsync(A.p, MSM_GUARD_BYTE, ws.total, stream));
  // the previous launch sequence on this workspace (of either route) left its counter region zero: no memset when this
  // one's fits in it
  const bool zeroed = !guard && lease.clean_bytes >= ws.zero_bytes && A.clean_off == ws.off_misc;
  if (int rc = launched(launch((char*)A.p, zeroed), label); rc != H2_OK) return rc;
  if (guard) {
    if (int rc = msm_guard_inspect(ws, (char*)A.p, stream, m, guard_what); rc != H2_OK) return rc;
  } else {
    A.clean_off = ws.off_misc;
    A.clean_bytes = ws.zero_bytes;
  }
  if (int rc = finish((char*)A.p); rc != H2_OK) return rc;
  return lease.release();
}

// h2_profile_*: the event pair around the accumulate kernel of a launch of m columns of n scalars, or nulls (profiling
// off, or no event to be had)
static std::pair<hipEvent_t, hipEvent_t> msm_prof_events(DevCtx& c, size_t n, size_t m) {
  if (!g_h2.profiling) return {nullptr, nullptr};
  if (c.prof_used == c.prof_events.size()) {
    hipEvent_t a, b;
    if (hipEventCreate(&a) == hipSuccess && hipEventCreate(&b) == hipSuccess) c.prof_events.push_back({a, b});
  }
  if (c.prof_used == c.prof_events.size()) return {nullptr, nullptr};
  c.prof_alg_bytes += (double)m * (double)n * 96.0 + (double)m * 96.0;  // SURVEY.md 8(d) bytes_msm
  return c.prof_events[c.prof_used++];
}

int msm_device_run(DevCtx& c, int curve, const BasesEntry& be, const void* d_scalars, size_t first_base, size_t n,
                   size_t col_stride, size_t m, void* d_out, bool affine_out, hipStream_t stream,
                   const BasesEntry* const* per_column) {
  if (msm_cols_per_launch(be.geom, n) == 0) return H2_EINVAL;   // a single column is already too long
  // columns with their own bases: one launch only (they must share the registered length, hence the geometry)
  const void* col_tables[MSM_MAX_MULTI];
  if (per_column) {
    if (m > MSM_MAX_MULTI) return H2_EINVAL;
    for (size_t j = 0; j < m; j++) {
      if (per_column[j]->n != be.n || per_column[j]->curve != be.curve) return H2_EINVAL;
      col_tables[j] = (const char*)per_column[j]->table[ctx_index(&c)] + first_base * 64;
    }
  }
  const size_t out_sz = affine_out ? 64 : 96;
  const CurveOps* ops = ops_of(curve);
  // the table rows of bases first_base ...: entries are w * n_bases + i relative to this pointer
  const char* table = (const char*)be.table[ctx_index(&c)] + first_base * 64;
  for (size_t j0 = 0; j0 < m;) {
    const MsmGroupPlan plan = msm_plan_group(be.geom, be.n, n, m - j0, col_stride, g_knobs.msm_guard, g_knobs.sort2_pack);
    const MsmWorkspace& ws = plan.ws;
    const size_t mm = plan.cols;
    if (per_column && mm < m) return H2_EINVAL;
    if (ws.E >= (1ull << 31) || ws.K >= (1ull << 31)) return H2_EINVAL;
    if (c.tail_wanted && !c.tail_event) H2_TRY(hipEventCreateWithFlags(&c.tail_event, hipEventDisableTiming));
    void* dst = (char*)d_out + j0 * out_sz;
    int rc = msm_run_group(
        c, stream, plan, "msm", "msm_launch", mm, ws.sort2 ? " two-level sort" : ws.staged ? " staged scatter" : " direct scatter",
        [&](char* ws_base, bool zeroed) {
          const auto [ev0, ev1] = msm_prof_events(c, n, mm);
          hipError_t e = ops->msm_launch(table, per_column ? col_tables : nullptr, (uint32_t)be.n,
                                         (const char*)d_scalars + j0 * col_stride * 32, n, col_stride, mm, be.geom, ws_base, ws, stream,
                                         ev0, ev1, (c.tail_wanted && !ev1) ? c.tail_event : nullptr, affine_out ? nullptr : dst, zeroed);
          c.tail_recorded = c.tail_wanted;
          c.tail_wait = ev1 ? ev1 : c.tail_event;
          return e;
        },
        [&](char* ws_base) {
          return affine_out ? launched(ops->to_affine(ws_base + ws.off_tree2, dst, (uint32_t)mm, stream), "msm finish kernel") : H2_OK;
        });
    if (rc != H2_OK) return rc;
    j0 += mm;
  }
  return H2_OK;
}

// What msm_device_run would refuse with H2_EINVAL for m columns of n scalars on `be`, found on the host without enqueuing
// anything: the same plans, in the same groups.  For a caller that enqueues work of its own in front of the MSM.
static int msm_device_plan_check(const BasesEntry& be, size_t n, size_t col_stride, size_t m) {
  if (msm_cols_per_launch(be.geom, n) == 0) return H2_EINVAL;
  for (size_t j0 = 0; j0 < m;) {
    const MsmGroupPlan plan = msm_plan_group(be.geom, be.n, n, m - j0, col_stride, g_knobs.msm_guard, g_knobs.sort2_pack);
    if (plan.cols == 0 || plan.ws.E >= (1ull << 31) || plan.ws.K >= (1ull << 31)) return H2_EINVAL;
    j0 += plan.cols;
  }
  return H2_OK;
}

// ---- table-free MSM over the caller's points (h2_msm_points.hpp) ---------------------------------------------------
// arguments checked by the caller; n >= 1, m >= 1
static int msm_points_run(DevCtx& c, int curve, const void* d_points, const void* d_scalars, size_t n, size_t col_stride,
                          size_t m, void* d_out, hipStream_t stream) {
  const CurveOps* ops = ops_of(curve);
  if (n < g_knobs.points_small_max) {
    // short inputs: one quad per term, m jobs side by side in groups of MSM_SMALL_MAX; the partials live in the MSM workspace
    const size_t blocks = (n + 15) / 16, work = MSM_SMALL_MAX * (blocks * (XYZZ29_WORDS * 4) + 4);
    for (size_t j0 = 0; j0 < m; j0 += MSM_SMALL_MAX) {
      const uint32_t count = (uint32_t)std::min<size_t>(MSM_SMALL_MAX, m - j0);
      ArenaLease lease(c.msm_ws.of(stream), work, stream);
      if (lease.rc != H2_OK) return lease.rc;
      const void* pts[MSM_SMALL_MAX];
      const void* sc[MSM_SMALL_MAX];
      uint32_t len[MSM_SMALL_MAX];
      for (uint32_t j = 0; j < count; j++) {
        pts[j] = d_points;
        sc[j] = (const char*)d_scalars + (j0 + j) * col_stride * 32;
        len[j] = (uint32_t)n;
      }
      if (int rc = launched(ops->msm_small(pts, sc, len, count, lease.a.p, (char*)d_out + j0 * 96, stream), "msm_small_kernel"); rc != H2_OK)
        return rc;
      if (int rc = lease.release(); rc != H2_OK) return rc;
    }
    return H2_OK;
  }
  const MsmGeom g = msm_points_geometry(n, ops->scalar_bits);
  for (size_t j0 = 0; j0 < m;) {
    const MsmGroupPlan plan = msm_points_plan_group(g, n, m - j0, col_stride, g_knobs.msm_guard);
    const size_t mm = plan.cols;
    if (mm == 0) return H2_EINVAL;
    int rc = msm_run_group(
        c, stream, plan, "msm points", "msm_points_launch", mm, " points front",
        [&](char* ws_base, bool zeroed) {
          return ops->msm_points_launch(d_points, (const char*)d_scalars + j0 * col_stride * 32, n, col_stride, mm, g, ws_base, plan.ws,
                                        stream, (char*)d_out + j0 * 96, zeroed);
        },
        [](char*) { return (int)H2_OK; });
    if (rc != H2_OK) return rc;
    j0 += mm;
  }
  return H2_OK;
}

// ---- NTT -----------------------------------------------------------------------------------
static int get_twiddles(DevCtx& c, const CurveOps* ops, const uint64_t omega[4], uint32_t log_n, const uint64_t* scale,
                        const void** out) {
  for (auto& t : c.twiddles) {
    if (t.field == ops->scalar_field_id && t.log_n == log_n && memcmp(t.omega, omega, 32) == 0 && t.scaled == (scale != nullptr) &&
        (!scale || memcmp(t.scale, scale, 32) == 0)) {
      t.stamp = ++c.stamp;
      *out = t.tw;
      return H2_OK;
    }
  }
  if (c.twiddles.size() >= 16) {  // evict the least recently used table
    size_t victim = 0;
    for (size_t i = 1; i < c.twiddles.size(); i++)
      if (c.twiddles[i].stamp < c.twiddles[victim].stamp) victim = i;
    H2_TRY(hipDeviceSynchronize());
    (void)hipFree(c.twiddles[victim].tw);
    c.twiddles.erase(c.twiddles.begin() + victim);
  }
  TwiddleEntry te{};
  te.field = ops->scalar_field_id;
  te.log_n = log_n;
  memcpy(te.omega, omega, 32);
  te.scaled = scale != nullptr;
  if (scale) memcpy(te.scale, scale, 32);
  if (int rc = device_alloc(&te.tw, ops->ntt_table_bytes(log_n), "twiddles"); rc != H2_OK) return rc;
  DeviceBuffer owner(te.tw);      // until the table is in the cache
  // built on the library's stream and finished before anybody uses it: a table is shared by every later caller,
  // whatever stream they bring (once per (field, omega, log n, constant))
  hipError_t e = ops->ntt_twiddles(te.tw, omega, log_n, c.stream, scale);
  if (e == hipSuccess) e = hipStreamSynchronize(c.stream);
  if (e != hipSuccess) return dev_fail(e, "ntt_build_tables");
  (void)owner.release();
  te.stamp = ++c.stamp;
  c.twiddles.push_back(te);
  *out = te.tw;
  return H2_OK;
}

// One transform launch sequence of m columns of 2^log_n: the tables of (omega, log_n[, table_scale]) -- none for one
// element -- and, for a two-pass plan, the second buffer on `stream` for as long as launch(tables, scratch) -> hipError_t
// uses it; `what` names the launch in an error
template <class Launch>
static int ntt_run(DevCtx& c, const CurveOps* ops, const uint64_t omega[4], uint32_t log_n, const uint64_t* table_scale, size_t m,
                   hipStream_t stream, const char* what, Launch&& launch) {
  const void* tw = nullptr;
  if (log_n > 0)
    if (int rc = get_twiddles(c, ops, omega, log_n, table_scale, &tw); rc != H2_OK) return rc;
  std::optional<ArenaLease> A;
  if (ntt_make_plan(log_n).npass > 1) {
    A.emplace(c.ntt_ws.of(stream), m * ((size_t)32 << log_n), stream);
    if (A->rc != H2_OK) return A->rc;
  }
  if (int rc = launched(launch(tw, A ? A->a.p : nullptr), what); rc != H2_OK) return rc;
  return A ? A->release() : H2_OK;
}

int ntt_enqueue(DevCtx& c, int curve, void* d_a, size_t m, const uint64_t omega[4], uint32_t log_n, hipStream_t stream,
                const uint64_t* scale) {
  const CurveOps* ops = ops_of(curve);
  if (!ops) return H2_EINVAL;
  // a constant that rides in the inter-pass twiddles needs tables built with it
  return ntt_run(c, ops, omega, log_n, (scale && ops->ntt_scale_in_table(log_n)) ? scale : nullptr, m, stream, "ntt_launch",
                 [&](const void* tw, void* scratch) { return ops->ntt_launch(d_a, scratch, tw, log_n, m, stream, scale); });
}

int coeff_to_extended_enqueue(DevCtx& c, int curve, const void* d_coeff, size_t col_stride, uint32_t log_n, size_t m,
                              const uint64_t zeta[4], const uint64_t ext_omega[4], uint32_t ext_log_n, void* d_out,
                              hipStream_t stream) {
  const CurveOps* ops = ops_of(curve);
  if (!ops) return H2_EINVAL;
  // pass 0 writes the second buffer; the padded source column never exists
  return ntt_run(c, ops, ext_omega, ext_log_n, nullptr, m, stream, "ntt_extend_launch", [&](const void* tw, void* scratch) {
    return ops->ntt_extend_launch(d_coeff, col_stride, log_n, zeta, d_out, scratch, tw, ext_log_n, m, stream);
  });
}

int extended_to_coeff_enqueue(DevCtx& c, int curve, const void* d_ext, uint32_t ext_log_n, size_t m,
                              const uint64_t ext_omega_inv[4], const uint64_t scale[4], const uint64_t zeta_inv[4], const void* d_t,
                              size_t t_period, void* d_out, size_t out_len, size_t out_stride, hipStream_t stream) {
  const CurveOps* ops = ops_of(curve);
  if (!ops) return H2_EINVAL;
  if (m == 0 || out_len == 0) return H2_OK;
  // ntt_enqueue's tables for the same (omega, log n, scale); pass 0 writes the second buffer: the source is only read
  return ntt_run(c, ops, ext_omega_inv, ext_log_n, ops->ntt_scale_in_table(ext_log_n) ? scale : nullptr, m, stream, "ntt_coeff_launch",
                 [&](const void* tw, void* scratch) {
                   return ops->ntt_coeff_launch(d_ext, d_t, t_period, scale, zeta_inv, d_out, out_len, out_stride, scratch, tw, ext_log_n,
                                                m, stream);
                 });
}

int poly_eval_enqueue(DevCtx& c, int curve, const void* const* d_polys, size_t n, const uint64_t* points, size_t q, void* d_out,
                      hipStream_t stream) {
  const CurveOps* ops = ops_of(curve);
  if (!ops || n == 0 || n > POLY_EVAL_MAX_N || q == 0) return H2_EINVAL;
  // jobs per launch sequence: grid.y, and what keeps the group's tile values under POLY_EVAL_WS_CAP
  const size_t per_job = poly_eval_ws_bytes(1, n);
  const size_t group = std::min<size_t>({q, (size_t)65535, std::max<size_t>(1, POLY_EVAL_WS_CAP / per_job)});
  const size_t table_bytes = h2_align256(q * sizeof(PolyEvalJob));
  ArenaLease A(c.div_ws, table_bytes + poly_eval_ws_bytes(group, n), stream);
  if (A.rc != H2_OK) return A.rc;
  std::vector<PolyEvalJob> table(q);
  for (size_t t = 0; t < q; t++) {
    table[t].poly = d_polys[t];
    memcpy(table[t].point, points + 4 * t, 32);
  }
  // a pageable source: the runtime has read `table` when the call returns (it stages the bytes or waits for the copy)
  H2_TRY(hipMemcpyAsync(A.a.p, table.data(), q * sizeof(PolyEvalJob), hipMemcpyHostToDevice, stream));
  const PolyEvalJob* d_jobs = (const PolyEvalJob*)A.a.p;
  void* ws = (char*)A.a.p + table_bytes;
  for (size_t t0 = 0; t0 < q; t0 += group) {             // the groups share `ws`: the stream runs them in order
    const size_t cnt = std::min(group, q - t0);
    if (int rc = launched(ops->poly_eval(d_jobs + t0, (uint32_t)cnt, n, ws, (char*)d_out + 32 * t0, stream), "poly_eval kernels"); rc != H2_OK)
      return rc;
  }
  return A.release();
}

// the three by the curve's scalar field
#define H2_BY_SCALAR_FIELD(curve, call)                          \
  ((curve) == H2_BN254    ? call<BN254_CURVE::Scalar>            \
   : (curve) == H2_PALLAS ? call<PALLAS_CURVE::Scalar>           \
                          : call<VESTA_CURVE::Scalar>)

// permutation_product_enqueue's tables (h2_permutation.hpp) at `out`, laid out by w: beta_p delta^j once per instance and
// column, the challenges, and omega^(run 2^b)
template <class FP>
static void perm_fill_tables(const PermWorkspace& w, const void* const* d_values, const void* const* d_sigma, size_t n_cols, size_t m,
                             const uint64_t* beta, const uint64_t* gamma, const uint64_t omega[4], const uint64_t delta[4], char* out) {
  using H = HF<FP>;
  PermColumn* cols = (PermColumn*)(out + w.off_columns);
  PermChallenge* ch = (PermChallenge*)(out + w.off_challenges);
  const H d = H::from_mont_limbs(delta);
  for (size_t p = 0; p < m; p++) {
    H bd = H::from_mont_limbs(beta + 4 * p);
    memcpy(ch[p].beta, beta + 4 * p, 32);
    memcpy(ch[p].gamma, gamma + 4 * p, 32);
    for (size_t j = 0; j < n_cols; j++) {
      PermColumn& c = cols[p * n_cols + j];
      c.value = d_values[p * n_cols + j];
      c.sigma = d_sigma[j];
      uint64_t limbs[4];
      bd.mont_limbs(limbs);
      memcpy(c.beta_delta, limbs, 32);
      bd = bd * d;
    }
  }
  H pw = H::from_mont_limbs(omega);
  for (int r = 1; r < perm_run(); r <<= 1) pw = pw.sqr();
  for (int b = 0; b < PERM_POW_BITS; b++) {
    uint64_t limbs[4];
    pw.mont_limbs(limbs);
    memcpy(out + w.off_powers + 32 * (size_t)b, limbs, 32);
    pw = pw.sqr();
  }
}

int permutation_product_enqueue(DevCtx& c, int curve, const void* const* d_values, const void* const* d_sigma, size_t n_cols, size_t chunk_len,
                                size_t u, size_t m, const uint64_t* beta, const uint64_t* gamma, const uint64_t omega[4],
                                const uint64_t delta[4], void* d_z, size_t col_stride, hipStream_t stream) {
  const CurveOps* ops = ops_of(curve);
  if (!ops || n_cols == 0 || chunk_len == 0 || m == 0) return H2_EINVAL;
  const size_t S = (n_cols - 1) / chunk_len + 1;
  const size_t scan_group = std::min(m, PERM_SCAN_GROUP);
  const PermWorkspace ws = perm_workspace(u, n_cols, S, m, scan_group);
  if (const char* broken = perm_check(ws, u, n_cols, chunk_len, S, m, scan_group, col_stride, ws.total)) {
    g_h2.last_error = std::string("permutation launch geometry: ") + broken;
    return H2_EDEVICE;
  }
  ArenaLease A(c.div_ws, ws.total, stream);
  if (A.rc != H2_OK) return A.rc;
  if (const char* broken = perm_check(ws, u, n_cols, chunk_len, S, m, scan_group, col_stride, A.a.bytes)) {   // the arena the lease handed out
    g_h2.last_error = std::string("permutation launch geometry: ") + broken;
    return H2_EDEVICE;
  }
  std::vector<char> tables(ws.off_scan);
  H2_BY_SCALAR_FIELD(curve, perm_fill_tables)(ws, d_values, d_sigma, n_cols, m, beta, gamma, omega, delta, tables.data());
  // a pageable source: the runtime has read `tables` when the call returns (it stages the bytes or waits for the copy)
  H2_TRY(hipMemcpyAsync(A.a.p, tables.data(), tables.size(), hipMemcpyHostToDevice, stream));
  for (size_t p0 = 0; p0 < m; p0 += PERM_RATIO_GROUP)
    if (int rc = launched(ops->perm_ratio(ws, (char*)A.a.p, p0, std::min(PERM_RATIO_GROUP, m - p0), u, n_cols, chunk_len, S, omega, d_z,
                                          col_stride, stream),
                          "perm_ratio_kernel");
        rc != H2_OK)
      return rc;
  for (size_t p0 = 0; u && p0 < m; p0 += scan_group)       // the groups share the scan values: the stream runs them in order
    if (int rc = launched(ops->perm_scan(ws, (char*)A.a.p, p0, std::min(scan_group, m - p0), u, S, d_z, col_stride, stream),
                          "permutation scan kernels");
        rc != H2_OK)
      return rc;
  return A.release();
}

}  // namespace h2

namespace {

// every *_device entry point: the library lock, the context of the current device, and the stream the work goes to
struct Call {
  std::lock_guard<std::recursive_mutex> lk{g_h2_mu};
  DevCtx* c = nullptr;
  hipStream_t stream = nullptr;
  int rc = H2_OK;
  Call(void* stream_) {
    if (!g_h2.ready) { rc = H2_ENOTINIT; return; }
    c = ctx_current();
    if (!c) { rc = H2_EINVAL; g_h2.last_error = "no h2 context on the current HIP device"; return; }
    stream = stream_ ? (hipStream_t)stream_ : c->stream;
  }
};

int init_devices(int n, const int* ids) {
  if (g_h2.ready) {
    if ((size_t)n != g_h2.ctx.size()) return H2_EINVAL;
    for (int i = 0; i < n; i++)
      if (g_h2.ctx[i].device != ids[i]) return H2_EINVAL;
    return H2_OK;
  }
  int count = 0;
  hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess || count == 0) {
    (void)hipGetLastError();
    g_h2.last_error = "no HIP device available";
    return H2_EDEVICE;
  }
  for (int i = 0; i < n; i++)
    if (ids[i] < 0 || ids[i] >= count) return H2_EINVAL;
  int prev = 0;
  (void)hipGetDevice(&prev);
  g_h2.ctx.assign((size_t)n, DevCtx{});
  for (int i = 0; i < n; i++) {
    DevCtx& c = g_h2.ctx[i];
    c.device = ids[i];
    H2_TRY(hipSetDevice(ids[i]));
    // a BLOCKING stream on purpose: callers that pass stream = NULL (e.g. PyTorch's legacy default stream)
    // get work that is ordered against the null stream, so their own copies / kernels see finished results
    H2_TRY(hipStreamCreateWithFlags(&c.stream, hipStreamDefault));
    for (int cv = 0; cv < 3; cv++) H2_TRY(ops_of(cv)->kernel_setup());
  }
  // one context: stay on its device (h2_init(device) has always left the process there); several: back to where we were
  H2_TRY(hipSetDevice(n == 1 ? ids[0] : prev));
  g_h2.ready = true;
  return H2_OK;
}

// m Jacobian points (96 B, Montgomery limbs) -> m affine points (64 B, identity = (0, 0)) on the host, the m inversions
// folded into one: the one-thread-per-point device kernel this replaces took 0.35 ms of pure latency per call
template <class FP>
void jac_to_affine_host(const uint8_t* jac, size_t m, uint8_t* out) {
  using H = HF<FP>;
  std::vector<H> z(m), pre(m);
  H acc = H::one();
  for (size_t j = 0; j < m; j++) {
    z[j] = H::from_mont_limbs(jac + 96 * j + 64);
    pre[j] = acc;
    if (!z[j].is_zero()) acc *= z[j];
  }
  H inv = acc.inv();
  for (size_t j = m; j-- > 0;) {
    uint8_t* o = out + 64 * j;
    if (z[j].is_zero()) {
      memset(o, 0, 64);
      continue;
    }
    const H zi = inv * pre[j], zi2 = zi.sqr();
    inv *= z[j];
    const H x = H::from_mont_limbs(jac + 96 * j) * zi2, y = H::from_mont_limbs(jac + 96 * j + 32) * zi2 * zi;
    memcpy(o, x.v.v, 32);
    memcpy(o + 32, y.v.v, 32);
  }
}
void jac_to_affine_host(int curve, const uint8_t* jac, size_t m, uint8_t* out) {
  if (curve == H2_BN254) jac_to_affine_host<BN254_FQ>(jac, m, out);
  else if (curve == H2_PALLAS) jac_to_affine_host<PASTA_FP>(jac, m, out);
  else jac_to_affine_host<PASTA_FQ>(jac, m, out);
}

// Host-pointer MSMs.  With several contexts (h2_init_devices) a batch is sharded by column, column j -> context
// j mod G, and a single long MSM by contiguous point range with the G partial sums added on context 0
// (SURVEY.md section 8(e)); every context works on its own stream, the host waits once at the end.
int msm_host(h2_curve_t curve, uint64_t handle, const uint64_t* const* cols, size_t n, size_t m, uint64_t* out,
                    bool affine_out) {
  const BasesEntry* be = nullptr;
  int rc = msm_common_checks((int)curve, handle, 0, n, m, &be);
  if (rc != H2_OK) return rc;
  if (!out || !cols) return H2_EINVAL;
  const size_t out_sz = affine_out ? 64 : 96;
  if (n == 0) {
    memset(out, 0, m * out_sz);
    return H2_OK;
  }
  for (size_t j = 0; j < m; j++)
    if (!cols[j]) return H2_EINVAL;
  const size_t G = g_h2.ctx.size();
  const size_t col_bytes = n * 32;
  if (m == 1 && G > 1 && n >= 4096 * G) {
    // point-range split of one MSM: context g takes bases [lo_g, hi_g)
    std::vector<uint64_t> partial(G * 12);
    std::vector<std::optional<ArenaLease>> stages(G);
    for (size_t g = 0; g < G; g++) {
      DevCtx& c = g_h2.ctx[g];
      DeviceGuard dg(c.device);
      const size_t lo = n * g / G, hi = n * (g + 1) / G, cnt = hi - lo;
      const size_t res_off = h2_align256(cnt * 32);
      if (int st = stages[g].emplace(c.stage, res_off + 96, c.stream).rc; st != H2_OK) return st;
      H2_TRY(hipMemcpyAsync(c.stage.p, (const char*)cols[0] + lo * 32, cnt * 32, hipMemcpyHostToDevice, c.stream));
      void* d_res = (char*)c.stage.p + res_off;
      rc = msm_device_run(c, (int)curve, *be, c.stage.p, lo, cnt, cnt, 1, d_res, false, c.stream);
      if (rc != H2_OK) return rc;
      H2_TRY(hipMemcpyAsync(&partial[12 * g], d_res, 96, hipMemcpyDeviceToHost, c.stream));
    }
    for (size_t g = 0; g < G; g++) {
      DeviceGuard dg(g_h2.ctx[g].device);
      if (int st = stages[g]->wait(); st != H2_OK) return st;
    }
    // add the G partial sums on context 0 (they are 96 bytes each)
    DevCtx& c = g_h2.ctx[0];
    DeviceGuard dg(c.device);
    const size_t res_off = h2_align256(G * 96);
    ArenaLease stage(c.stage, res_off + 96, c.stream);
    if (stage.rc != H2_OK) return stage.rc;
    H2_TRY(hipMemcpyAsync(c.stage.p, partial.data(), G * 96, hipMemcpyHostToDevice, c.stream));
    void* d_res = (char*)c.stage.p + res_off;
    if (int st = launched(ops_of((int)curve)->points_sum(c.stage.p, d_res, (uint32_t)G, 1, c.stream), "points_sum_kernel"); st != H2_OK)
      return st;
    if (affine_out) return H2_EINVAL;   // not reached: h2_msm asks for Jacobian
    H2_TRY(hipMemcpyAsync(out, d_res, 96, hipMemcpyDeviceToHost, c.stream));
    return stage.wait();
  }
  // column sharding: context g takes columns g, g + G, ...; the results come back as Jacobian points and are
  // normalised on the host when the caller wants affine ones
  std::vector<uint8_t> jac(affine_out ? m * 96 : 0);
  uint8_t* dst = affine_out ? jac.data() : (uint8_t*)out;
  std::vector<std::optional<ArenaLease>> stages(G);
  for (size_t g = 0; g < G && g < m; g++) {
    DevCtx& c = g_h2.ctx[g];
    DeviceGuard dg(c.device);
    const size_t mine = (m - g + G - 1) / G;
    const size_t res_off = h2_align256(mine * col_bytes);
    if (int st = stages[g].emplace(c.stage, res_off + mine * 96, c.stream).rc; st != H2_OK) return st;
    for (size_t i = 0; i < mine; i++)
      H2_TRY(hipMemcpyAsync((char*)c.stage.p + i * col_bytes, cols[g + i * G], col_bytes, hipMemcpyHostToDevice,
                            c.stream));
    void* d_res = (char*)c.stage.p + res_off;
    rc = msm_device_run(c, (int)curve, *be, c.stage.p, 0, n, n, mine, d_res, false, c.stream);
    if (rc != H2_OK) return rc;
    if (G == 1) {
      H2_TRY(hipMemcpyAsync(dst, d_res, mine * 96, hipMemcpyDeviceToHost, c.stream));
    } else {
      for (size_t i = 0; i < mine; i++)
        H2_TRY(hipMemcpyAsync(dst + (g + i * G) * 96, (char*)d_res + i * 96, 96, hipMemcpyDeviceToHost, c.stream));
    }
  }
  for (size_t g = 0; g < G && g < m; g++) {
    DeviceGuard dg(g_h2.ctx[g].device);
    if (int st = stages[g]->wait(); st != H2_OK) return st;
  }
  if (affine_out) jac_to_affine_host((int)curve, jac.data(), m, (uint8_t*)out);
  return H2_OK;
}

// ---- expressions over resident columns (h2_expr_program.hpp compiles, h2_expr_kernel.hpp interprets) ----------------------
constexpr size_t EXPR_TABLE_CAP = (size_t)256 << 20;   // bytes of constant tables one group of instances may take
constexpr size_t EXPR_MAX_COUNT = (size_t)1 << 20;     // nodes, constants, variables
constexpr size_t EXPR_MAX_INSTANCES = (size_t)1 << 30;

// 4 x u64 Montgomery limbs: the integer they hold is below p
template <class FP>
bool mont_canonical(const uint64_t* v) {
  for (int i = 3; i >= 0; i--) {
    const uint64_t pw = (uint64_t)FP::P(2 * i) | ((uint64_t)FP::P(2 * i + 1) << 32);
    if (v[i] != pw) return v[i] < pw;
  }
  return false;
}
// the API form x 2^256 -> the kernel's working form x 2^261 (R' = 2^261): five doublings
template <class FP>
void expr_working_form(const uint64_t* api, uint64_t* out) {
  HF<FP> c = HF<FP>::from_mont_limbs(api);
  for (int t = 0; t < 5; t++) c = c + c;
  c.mont_limbs(out);
}

template <class FP>
void expr_compile_t(const h2_expr_node_t* nodes, size_t n_nodes, const uint64_t* consts, size_t n_consts, uint32_t n_cols,
                    uint32_t n_vars, ExprEntry& e) {
  using product::fail;
  std::vector<HF<FP>> cs(n_consts);
  for (size_t j = 0; j < n_consts; j++) {
    if (!mont_canonical<FP>(consts + 4 * j)) fail(H2_EINVAL, "expr: constant not canonical");
    cs[j] = HF<FP>::from_mont_limbs(consts + 4 * j);
  }
  static_assert(sizeof(h2_expr_node_t) == 16, "four i32 per node");
  product::ExprProgramT<FP> X;
  product::program_from_nodes<FP>(X, (const int32_t*)nodes, n_nodes, cs, n_cols, n_vars, true, &e.var_slot);
  const size_t lds = product::expr_lds_bytes(X);       // H2_EINVAL past what one workgroup may hold
  const std::vector<uint8_t> rep = X.report();
  uint32_t st[6];
  memcpy(st, rep.data(), 24);
  e.info = h2_expr_info_t{0, st[0], st[1], st[2], st[3], st[4], st[5], n_cols, n_vars, (uint32_t)lds, 0, 0};
  bool any = false;
  for (auto& ins : X.code)
    for (uint32_t w : {ins.a, ins.b})
      if ((w & (3u << 30)) == pk::X_COL) {
        const int32_t rot = (int32_t)(w & 0xFFu) - 128;
        e.info.min_rot = any ? std::min(e.info.min_rot, rot) : rot;
        e.info.max_rot = any ? std::max(e.info.max_rot, rot) : rot;
        any = true;
      }
  e.code.resize(3 * X.code.size());
  memcpy(e.code.data(), X.code.data(), X.code.size() * sizeof(pk::XInstr));
  e.table.resize(4 * X.consts.size());
  for (size_t j = 0; j < X.consts.size(); j++) {
    uint64_t api[4];
    X.consts[j].mont_limbs(api);
    expr_working_form<FP>(api, e.table.data() + 4 * j);
  }
  e.dump = X.report_with_table();
  const size_t at = e.dump.size();
  e.dump.resize(at + 4 * e.var_slot.size());
  if (!e.var_slot.empty()) memcpy(e.dump.data() + at, e.var_slot.data(), 4 * e.var_slot.size());
}

// the constant tables of instances [p0, p0 + cnt): the program's own table with the instance's variables in their slots
template <class FP>
void expr_fill_tables(const ExprEntry& e, const uint64_t* vars, size_t p0, size_t cnt, uint64_t* out) {
  const size_t words = e.table.size(), nv = e.var_slot.size();
  for (size_t p = 0; p < cnt; p++) {
    uint64_t* t = out + p * words;
    memcpy(t, e.table.data(), words * 8);
    for (size_t v = 0; v < nv; v++) expr_working_form<FP>(vars + 4 * ((p0 + p) * nv + v), t + 4 * (size_t)e.var_slot[v]);
  }
}


// ---- Poseidon (h2_poseidon_host.hpp generates the constants, h2_poseidon.hpp holds the kernels) --------------------------
constexpr size_t POSEIDON_TABLE_SLOTS = 8;

bool poseidon_rounds_ok(uint32_t r_f, uint32_t r_p) {
  return r_f >= 2 && !(r_f & 1) && r_f <= POSEIDON_MAX_ROUNDS && r_p <= POSEIDON_MAX_ROUNDS && r_f + r_p <= POSEIDON_MAX_ROUNDS;
}
// ConstantLength<len>'s capacity word len 2^64 as Montgomery limbs
template <class FP>
void poseidon_capacity_t(uint64_t len, uint64_t out[4]) {
  const HF<FP> two32 = HF<FP>::from_u64(1ull << 32);
  (HF<FP>::from_u64(len) * two32 * two32).mont_limbs(out);
}
bool poseidon_width_ok(uint32_t width) { return width == 3 || width == 5 || width == 9; }
// (r_f + r_p) * width round constants, then the width x width MDS row-major, as Montgomery limbs; with `sparse` the sparse
// part of the kernels' table behind them (poseidon_table_elems in all; widths 5 and 9).  False when the partial rounds do
// not factor
template <class FP>
bool poseidon_wide_constants_t(uint32_t width, uint32_t r_f, uint32_t r_p, bool sparse, uint64_t* out) {
  const poseidon::WideConstants<FP> k = poseidon::generate_wide<FP>((int)width, (int)r_f, (int)r_p);
  for (auto& c : k.rcs) { c.mont_limbs(out); out += 4; }
  for (auto& m : k.mds) { m.mont_limbs(out); out += 4; }
  if (!sparse) return true;
  poseidon::SparseRounds<FP> sp;
  if (!poseidon::factor_partial_rounds(k, (int)r_f, (int)r_p, &sp)) return false;
  for (auto* part : {&sp.pre, &sp.d0, &sp.rounds})
    for (auto& e : *part) { e.mont_limbs(out); out += 4; }
  HF<FP>::one().mont_limbs(out);
  return true;
}
// The table of (curve, width, r_f, r_p) on context c, built by its first user.  A table is uploaded on the library's stream
// and finished before anybody reads it, as the NTT tables are: every later caller shares it whatever stream it brings.  The
// cache keeps POSEIDON_TABLE_SLOTS tables; the oldest one is dropped for a ninth, after the device has run everything
// enqueued so far -- work that still reads the dropped table is finished before the memory is freed.
int poseidon_table_get(DevCtx& c, int curve, uint32_t width, uint32_t r_f, uint32_t r_p, const void** out) {
  const CurveOps* ops = ops_of(curve);
  for (auto& t : c.poseidon_tables)
    if (t.field == ops->scalar_field_id && t.width == width && t.r_f == r_f && t.r_p == r_p) {
      *out = t.d;
      return H2_OK;
    }
  if (c.poseidon_tables.size() >= POSEIDON_TABLE_SLOTS) {
    H2_TRY(hipDeviceSynchronize());
    (void)hipFree(c.poseidon_tables.front().d);
    c.poseidon_tables.erase(c.poseidon_tables.begin());
  }
  const size_t elems = poseidon_table_elems(width, r_f, r_p);
  std::vector<uint64_t> api(4 * elems);
  if (!H2_BY_SCALAR_FIELD(curve, poseidon_wide_constants_t)(width, r_f, r_p, width != 3, api.data())) {
    g_h2.last_error = "poseidon: the partial rounds of this instance do not factor";
    return H2_EINVAL;
  }
  std::vector<int32_t> table(9 * elems);
  poseidon_ops_of(curve)->table(api.data(), elems, table.data());
  PoseidonTable te{ops->scalar_field_id, width, r_f, r_p, nullptr};
  if (int rc = device_alloc(&te.d, table.size() * 4, "poseidon table"); rc != H2_OK) return rc;
  DeviceBuffer owner(te.d);      // until the table is in the cache
  hipError_t e = hipMemcpyAsync(te.d, table.data(), table.size() * 4, hipMemcpyHostToDevice, c.stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c.stream);
  if (e != hipSuccess) return dev_fail(e, "poseidon table upload");
  (void)owner.release();
  c.poseidon_tables.push_back(te);
  *out = te.d;
  return H2_OK;
}
// lanes from which a hash launch takes the single-chain products (h2_poseidon.hpp), unless a test knob fixes the form
size_t poseidon_chain_min_n() { return g_knobs.poseidon_form == 1 ? SIZE_MAX : g_knobs.poseidon_form == 2 ? 0 : POSEIDON_CHAIN_MIN_N; }
bool poseidon_dev_ptr(const void* p) { return p && !((uintptr_t)p & 15); }
bool poseidon_overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + b_bytes && y < x + a_bytes;
}

}  // namespace

bool h2::poseidon_wide_table_mont(int curve, uint32_t width, uint32_t r_f, uint32_t r_p, bool sparse, uint64_t* out) {
  return H2_BY_SCALAR_FIELD(curve, poseidon_wide_constants_t)(width, r_f, r_p, sparse, out);
}
void h2::poseidon_capacity_mont(int curve, uint64_t len, uint64_t out[4]) { H2_BY_SCALAR_FIELD(curve, poseidon_capacity_t)(len, out); }

// h2_transcript_challenge: Challenge255 of a 64-byte digest, Montgomery limbs
template <class FP>
static void transcript_reduce(const uint8_t digest[64], uint64_t out[4]) {
  HF<FP>::from_le_bytes_wide(digest).mont_limbs(out);
}

// count x 4 limbs, every element below the modulus?
template <class FP>
static bool ipa_canonical(const uint64_t* limbs, size_t count) {
  for (size_t i = 0; i < count; i++) {
    HF<FP> x;
    uint8_t b[32];
    memcpy(b, limbs + 4 * i, 32);
    if (!HF<FP>::from_le_bytes_canonical(b, &x)) return false;
  }
  return true;
}

extern "C" {

int h2_version(void) { return 1002; }

const char* h2_strerror(int s) {
  switch (s) {
    case H2_OK: return "ok";
    case H2_EINVAL: return "invalid argument (length / log_n mismatch, null pointer or unknown curve)";
    case H2_ENOMEM: return "out of memory";
    case H2_EDEVICE: return "HIP device error";
    case H2_EHANDLE: return "unknown bases handle";
    case H2_ENOTINIT: return "h2_init has not been called";
    case H2_EPROOF: return "proof or input rejected";
  }
  return "unknown status";
}

const char* h2_last_device_error(void) {
  std::lock_guard<std::recursive_mutex> lk(g_h2_mu);
  static thread_local std::string copy;
  copy = g_h2.last_error;
  return copy.c_str();
}

int h2_init(int device) {
  std::lock_guard<std::recursive_mutex> lk(g_h2_mu);
  return init_devices(1, &device);
}

int h2_init_devices(int n_devices, const int* device_ids) {
  std::lock_guard<std::recursive_mutex> lk(g_h2_mu);
  if (n_devices <= 0 || n_devices > 64 || !device_ids) return H2_EINVAL;
  return init_devices(n_devices, device_ids);
}

int h2_device_count(void) {
  std::lock_guard<std::recursive_mutex> lk(g_h2_mu);
  return g_h2.ready ? (int)g_h2.ctx.size() : H2_ENOTINIT;
}

void h2_prover_shutdown(void);   // h2_prover.hip: keys, params and cached blocks of the product surface

int h2_shutdown(void) {
  std::lock_guard<std::recursive_mutex> lk(g_h2_mu);
  if (!g_h2.ready) return H2_OK;
  h2_prover_shutdown();
  for (size_t i = 0; i < g_h2.ctx.size(); i++) {
    DevCtx& c = g_h2.ctx[i];
    DeviceGuard dg(c.device);
    (void)hipDeviceSynchronize();
    for (auto& kv : g_h2.bases)
      if (kv.second.table[i]) (void)hipFree(kv.second.table[i]);
    for (auto& t : c.twiddles) (void)hipFree(t.tw);
    for (auto& t : c.poseidon_tables) (void)hipFree(t.d);
    for (auto& kv : g_h2.exprs)
      if (i < kv.second.d_code.size() && kv.second.d_code[i]) (void)hipFree(kv.second.d_code[i]);
    for (Arena& a : c.msm_ws.slot) arena_free(a);
    for (Arena& a : c.ntt_ws.slot) arena_free(a);
    arena_free(c.stage);
    arena_free(c.div_ws);
    for (auto& pe : c.prof_events) {
      (void)hipEventDestroy(pe.first);
      (void)hipEventDestroy(pe.second);
    }
    if (c.shard_ev) (void)hipEventDestroy(c.shard_ev);
    if (c.side_stream) (void)hipStreamDestroy(c.side_stream);
    for (auto& e : c.side_ev)
      if (e) (void)hipEventDestroy(e);
    (void)hipStreamDestroy(c.stream);
  }
  g_h2.bases.clear();
  for (auto& kv : g_h2.exprs) kv.second.d_code.clear();      // the programs themselves are host state and stay
  g_h2.ctx.clear();
  g_h2.ready = false;
  return H2_OK;
}

int h2_bases_register_device(h2_curve_t curve, const void* d_affine, size_t n, uint64_t* handle_out) {
  Call k(nullptr);
  if (k.rc != H2_OK) return k.rc;
  // the caller's copy / kernel that produced d_affine may still be in flight on another stream
  H2_TRY(hipDeviceSynchronize());
  return register_device(*k.c, (int)curve, d_affine, n, handle_out);
}

int h2_bases_register(h2_curve_t curve, const uint64_t* affine, size_t n, uint64_t* handle_out) {
  std::lock_guard<std::recursive_mutex> lk(g_h2_mu);
  if (!g_h2.ready) return H2_ENOTINIT;
  if (!curve_ok((int)curve) || !affine || !handle_out || n == 0) return H2_EINVAL;
  DevCtx& c = g_h2.ctx[0];
  DeviceGuard dg(c.device);
  ArenaLease stage(c.stage, n * 64, c.stream);
  if (stage.rc != H2_OK) return stage.rc;
  H2_TRY(hipMemcpyAsync(c.stage.p, affine, n * 64, hipMemcpyHostToDevice, c.stream));
  return register_device(c, (int)curve, c.stage.p, n, handle_out);   // synchronises c.stream
}

int h2_bases_release(uint64_t handle) {
  std::lock_guard<std::recursive_mutex> lk(g_h2_mu);
  if (!g_h2.ready) return H2_ENOTINIT;
  auto it = g_h2.bases.find(handle);
  if (it == g_h2.bases.end()) return H2_EHANDLE;
  for (size_t i = 0; i < g_h2.ctx.size(); i++) {
    DeviceGuard dg(g_h2.ctx[i].device);
    (void)hipDeviceSynchronize();     // launches on caller streams may still read the table
    (void)hipFree(it->second.table[i]);
  }
  g_h2.bases.erase(it);
  return H2_OK;
}

int64_t h2_bases_len(uint64_t handle) {
  std::lock_guard<std::recursive_mutex> lk(g_h2_mu);
  if (!g_h2.ready) return H2_ENOTINIT;
  auto it = g_h2.bases.find(handle);
  if (it == g_h2.bases.end()) return H2_EHANDLE;
  return (int64_t)it->second.n;
}

int h2_msm_plan(uint64_t handle, h2_msm_plan_t* out) {
  std::lock_guard<std::recursive_mutex> lk(g_h2_mu);
  if (!g_h2.ready) return H2_ENOTINIT;
  if (!out) return H2_EINVAL;
  auto it = g_h2.bases.find(handle);
  if (it == g_h2.bases.end()) return H2_EHANDLE;
  out->window_bits = it->second.geom.c;
  out->windows = it->second.geom.W;
  out->buckets = it->second.geom.B;
  out->table_bytes = it->second.table_bytes;
  return H2_OK;
}

int h2_msm_device_range(h2_curve_t curve, uint64_t handle, const void* d_scalars, size_t first_base, size_t n,
                        size_t col_stride, size_t m, void* d_out_jac, void* stream_) {
  Call k(stream_);
  const BasesEntry* be = nullptr;
  int rc = msm_common_checks((int)curve, handle, first_base, n, m, &be);
  if (rc != H2_OK) return rc;
  if (!d_out_jac || (n && !d_scalars) || (m > 1 && col_stride < n)) return H2_EINVAL;
  if (k.rc != H2_OK) return k.rc;
  if (n == 0) {
    H2_TRY(hipMemsetAsync(d_out_jac, 0, m * 96, k.stream));
    return H2_OK;
  }
  return msm_device_run(*k.c, (int)curve, *be, d_scalars, first_base, n, col_stride, m, d_out_jac, false, k.stream);
}

int h2_msm_device_multi(h2_curve_t curve, const uint64_t* handles, const void* d_scalars, size_t first_base, size_t n,
                        size_t col_stride, size_t m, void* d_out_jac, void* stream_) {
  Call k(stream_);
  if (!handles || m == 0 || m > MSM_MAX_MULTI) return H2_EINVAL;
  const BasesEntry* bes[MSM_MAX_MULTI];
  for (size_t j = 0; j < m; j++) {
    int rc = msm_common_checks((int)curve, handles[j], first_base, n, m, &bes[j]);
    if (rc != H2_OK) return rc;
  }
  if (!d_out_jac || (n && !d_scalars) || (m > 1 && col_stride < n)) return H2_EINVAL;
  if (k.rc != H2_OK) return k.rc;
  if (n == 0) {
    H2_TRY(hipMemsetAsync(d_out_jac, 0, m * 96, k.stream));
    return H2_OK;
  }
  return msm_device_run(*k.c, (int)curve, *bes[0], d_scalars, first_base, n, col_stride, m, d_out_jac, false, k.stream, bes);
}

int h2_msm_device(h2_curve_t curve, uint64_t handle, const void* d_scalars, size_t n, size_t m, void* d_out_jac,
                  void* stream_) {
  return h2_msm_device_range(curve, handle, d_scalars, 0, n, n, m, d_out_jac, stream_);
}

int h2_stream_wait_msm_tail(void* stream_) {
  Call k(stream_);
  if (k.rc != H2_OK) return k.rc;
  if (k.c->tail_recorded && k.c->tail_wait) H2_TRY(hipStreamWaitEvent(k.stream, k.c->tail_wait, 0));
  k.c->tail_wanted = true;          // from now on every MSM of this context marks the end of its accumulate kernel
  return H2_OK;
}

int h2_points_sum_device(h2_curve_t curve, const void* d_in_jac, size_t groups, size_t count, void* d_out_jac,
                         void* stream_) {
  Call k(stream_);
  if (k.rc != H2_OK) return k.rc;
  if (!curve_ok((int)curve) || !d_in_jac || !d_out_jac || groups == 0 || groups > (1u << 20) || count > (1u << 24))
    return H2_EINVAL;
  if (count == 0) return H2_OK;
  return launched(ops_of((int)curve)->points_sum(d_in_jac, d_out_jac, (uint32_t)groups, (uint32_t)count, k.stream), "points_sum_kernel");
}

int h2_points_decompress_device(h2_curve_t curve, const void* d_compressed, size_t n, void* d_out_affine, void* d_status,
                                void* stream_) {
  Call k(stream_);
  if (k.rc != H2_OK) return k.rc;
  if (!curve_ok((int)curve) || !ops_of((int)curve)->points_decompress || n > (1u << 30)) return H2_EINVAL;
  if (n == 0) return H2_OK;
  // the kernel moves 16 bytes at a time
  if (!d_compressed || !d_out_affine || !d_status || ((uintptr_t)d_compressed & 15) || ((uintptr_t)d_out_affine & 15))
    return H2_EINVAL;
  return launched(ops_of((int)curve)->points_decompress(d_compressed, d_out_affine, d_status, (uint32_t)n, k.stream), "points_decompress_kernel");
}

// [a, a + la) and [b, b + lb) share bytes without being the same range
static bool partly_overlaps(const void* a, size_t la, const void* b, size_t lb) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  if (a0 == b0 && la == lb) return false;
  return a0 < b0 + lb && b0 < a0 + la;
}
static bool overlaps(const void* a, size_t la, const void* b, size_t lb) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + lb && b0 < a0 + la;
}

int h2_base_sqrt_device(h2_curve_t curve, const void* d_in, size_t n, void* d_out, void* d_status, void* stream_) {
  Call k(stream_);
  if (k.rc != H2_OK) return k.rc;
  if (!curve_ok((int)curve) || n > (1u << 30)) return H2_EINVAL;
  if (n == 0) return H2_OK;
  // the kernel moves 16 bytes at a time; the roots may replace the elements, nothing else may share bytes
  if (!d_in || !d_out || !d_status || ((uintptr_t)d_in & 15) || ((uintptr_t)d_out & 15)) return H2_EINVAL;
  if (partly_overlaps(d_in, n * 32, d_out, n * 32) || overlaps(d_status, n, d_in, n * 32) || overlaps(d_status, n, d_out, n * 32))
    return H2_EINVAL;
  return launched(ops_of((int)curve)->base_sqrt(d_in, d_out, d_status, (uint32_t)n, k.stream), "base_sqrt_kernel");
}

int h2_pasta_points_decompress_device(h2_curve_t curve, const void* d_compressed, size_t n, void* d_out_affine, void* d_status,
                                      void* stream_) {
  Call k(stream_);
  if (k.rc != H2_OK) return k.rc;
  if (!curve_ok((int)curve) || !ops_of((int)curve)->pasta_points_decompress || n > (1u << 30)) return H2_EINVAL;
  if (n == 0) return H2_OK;
  if (!d_compressed || !d_out_affine || !d_status || ((uintptr_t)d_compressed & 15) || ((uintptr_t)d_out_affine & 15))
    return H2_EINVAL;
  if (overlaps(d_compressed, n * 32, d_out_affine, n * 64) || overlaps(d_status, n, d_compressed, n * 32) ||
      overlaps(d_status, n, d_out_affine, n * 64))
    return H2_EINVAL;
  return launched(ops_of((int)curve)->pasta_points_decompress(d_compressed, d_out_affine, d_status, (uint32_t)n, k.stream),
                  "points_decompress_kernel");
}

int h2_msm(h2_curve_t curve, uint64_t handle, const uint64_t* scalars, size_t n, uint64_t out_jac[12]) {
  std::lock_guard<std::recursive_mutex> lk(g_h2_mu);
  if (n && !scalars) return H2_EINVAL;
  const uint64_t* cols[1] = {scalars ? scalars : (const uint64_t*)out_jac};
  return msm_host(curve, handle, cols, n, 1, out_jac, false);
}

int h2_msm_batch(h2_curve_t curve, uint64_t handle, const uint64_t* const* scalars, size_t n, size_t m,
                 uint64_t* out_affine) {
  std::lock_guard<std::recursive_mutex> lk(g_h2_mu);
  return msm_host(curve, handle, scalars, n, m, out_affine, true);
}

int h2_msm_points_plan(h2_curve_t curve, size_t n, h2_msm_points_plan_t* out) {
  std::lock_guard<std::recursive_mutex> lk(g_h2_mu);
  if (!curve_ok((int)curve) || !out || n > MSM_POINTS_MAX_N) return H2_EINVAL;
  const MsmGeom g = msm_points_geometry(n ? n : 1, ops_of((int)curve)->scalar_bits);
  memset(out, 0, sizeof *out);
  out->window_bits = g.c;
  out->windows = g.W;
  out->buckets = g.B;
  out->route = n < g_knobs.points_small_max ? 0u : 1u;
  out->scalar_bits = g.nbits;
  out->lds_bytes = (uint32_t)((size_t)g.W * g.B * 4);
  out->lds_limit = (uint32_t)MSM_POINTS_LDS_CAP;
  out->crossover = (uint64_t)g_knobs.points_small_max;
  out->max_n = (uint64_t)MSM_POINTS_MAX_N;
  for (uint32_t w = 0; w < g.W; w++) {
    out->width[w] = g.width[w];
    out->offset[w] = g.off[w];
  }
  return H2_OK;
}

int h2_msm_points_device(h2_curve_t curve, const void* d_points, const void* d_scalars, size_t n, size_t col_stride, size_t m,
                         void* d_out_jac, void* stream_) {
  Call k(stream_);
  if (k.rc != H2_OK) return k.rc;
  if (!curve_ok((int)curve) || col_stride < n || n > MSM_POINTS_MAX_N) return H2_EINVAL;
  if (((uintptr_t)d_points & 15) || ((uintptr_t)d_scalars & 15) || ((uintptr_t)d_out_jac & 15)) return H2_EINVAL;
  if (m > 0 && (!d_out_jac || (n > 0 && (!d_points || !d_scalars)))) return H2_EINVAL;
  if (m == 0) return H2_OK;
  if (n == 0) {
    H2_TRY(hipMemsetAsync(d_out_jac, 0, m * 96, k.stream));
    return H2_OK;
  }
  return msm_points_run(*k.c, (int)curve, d_points, d_scalars, n, col_stride, m, d_out_jac, k.stream);
}

int h2_msm_points(h2_curve_t curve, const uint64_t* points, const uint64_t* scalars, size_t n, uint64_t out_jac[12]) {
  Call k(nullptr);
  if (k.rc != H2_OK) return k.rc;
  if (!curve_ok((int)curve) || n > MSM_POINTS_MAX_N || !out_jac || (n > 0 && (!points || !scalars))) return H2_EINVAL;
  if (n == 0) {
    memset(out_jac, 0, 96);
    return H2_OK;
  }
  DevCtx& c = *k.c;
  const size_t off_sc = h2_align256(n * 64), off_res = off_sc + h2_align256(n * 32);
  ArenaLease stage(c.stage, off_res + 96, c.stream);
  if (stage.rc != H2_OK) return stage.rc;
  char* base = (char*)c.stage.p;
  H2_TRY(hipMemcpyAsync(base, points, n * 64, hipMemcpyHostToDevice, c.stream));
  H2_TRY(hipMemcpyAsync(base + off_sc, scalars, n * 32, hipMemcpyHostToDevice, c.stream));
  if (int rc = msm_points_run(c, (int)curve, base, base + off_sc, n, n, 1, base + off_res, c.stream); rc != H2_OK) return rc;
  H2_TRY(hipMemcpyAsync(out_jac, base + off_res, 96, hipMemcpyDeviceToHost, c.stream));
  return stage.wait();
}

int h2_srs_generate(h2_curve_t curve, const uint64_t s[4], size_t n, void* d_out_affine, void* stream_) {
  Call k(stream_);
  if (k.rc != H2_OK) return k.rc;
  const CurveOps* ops = ops_of((int)curve);
  if (!ops || !s || !d_out_affine || n == 0 || n >= (1ull << 32)) return H2_EINVAL;
  return launched(ops->srs_powers(d_out_affine, s, (uint32_t)n, k.stream), "srs_powers_kernel");
}

int h2_fixed_base_mul(h2_curve_t curve, const void* d_scalars, size_t n, void* d_out_affine, void* stream_) {
  Call k(stream_);
  if (k.rc != H2_OK) return k.rc;
  const CurveOps* ops = ops_of((int)curve);
  if (!ops || !d_scalars || !d_out_affine || n == 0 || n >= (1ull << 32)) return H2_EINVAL;
  return launched(ops->fixed_base_mul(d_out_affine, d_scalars, (uint32_t)n, k.stream), "fixed_base_mul_kernel");
}

int h2_profile_enable(int on) {
  std::lock_guard<std::recursive_mutex> lk(g_h2_mu);
  g_h2.profiling = on != 0;
  for (auto& c : g_h2.ctx) {
    c.prof_used = 0;
    c.prof_alg_bytes = 0;
  }
  return H2_OK;
}

int h2_profile_read(h2_profile_t* out) {
  std::lock_guard<std::recursive_mutex> lk(g_h2_mu);
  if (!out) return H2_EINVAL;
  double ms = 0, bytes = 0;
  uint64_t launches = 0;
  for (auto& c : g_h2.ctx) {
    DeviceGuard dg(c.device);
    for (size_t i = 0; i < c.prof_used; i++) {
      float t = 0;
      H2_TRY(hipEventSynchronize(c.prof_events[i].second));
      H2_TRY(hipEventElapsedTime(&t, c.prof_events[i].first, c.prof_events[i].second));
      ms += t;
    }
    launches += c.prof_used;
    bytes += c.prof_alg_bytes;
    c.prof_used = 0;
    c.prof_alg_bytes = 0;
  }
  out->launches = launches;
  out->kernel_ms = ms;
  out->algorithmic_bytes = bytes;
  return H2_OK;
}

int h2_ntt_device(h2_curve_t curve, void* d_a, size_t m, const uint64_t omega[4], uint32_t log_n, void* stream_) {
  Call k(stream_);
  if (k.rc != H2_OK) return k.rc;
  if (!curve_ok((int)curve) || !d_a || !omega || m == 0 || log_n > 30) return H2_EINVAL;
  if (log_n == 0) return H2_OK;
  return ntt_enqueue(*k.c, (int)curve, d_a, m, omega, log_n, k.stream);
}

int h2_ntt_scaled_device(h2_curve_t curve, void* d_a, size_t m, const uint64_t omega[4], uint32_t log_n,
                         const uint64_t scale[4], void* stream_) {
  Call k(stream_);
  if (k.rc != H2_OK) return k.rc;
  if (!curve_ok((int)curve) || !d_a || !omega || !scale || m == 0 || log_n > 30) return H2_EINVAL;
  if (log_n == 0) {
    return launched(ops_of((int)curve)->poly_scale(d_a, m, scale, k.stream), "poly_scale_kernel");
  }
  return ntt_enqueue(*k.c, (int)curve, d_a, m, omega, log_n, k.stream, scale);
}

int h2_coeff_to_extended_device(h2_curve_t curve, const void* d_coeff, size_t col_stride, uint32_t log_n, size_t m,
                                const uint64_t zeta[4], const uint64_t ext_omega[4], uint32_t ext_log_n, void* d_out,
                                void* stream_) {
  Call k(stream_);
  if (k.rc != H2_OK) return k.rc;
  if (!curve_ok((int)curve) || !zeta || !ext_omega || ext_log_n > 30 || ext_log_n < log_n) return H2_EINVAL;
  const size_t n = (size_t)1 << log_n, en = (size_t)1 << ext_log_n;
  if (col_stride < n) return H2_EINVAL;
  if (m == 0) return H2_OK;
  if (!d_coeff || !d_out || m > 65535) return H2_EINVAL;             // grid.y = column
  // [first byte, last byte) of what is read and of what is written
  const uintptr_t s0 = (uintptr_t)d_coeff, s1 = s0 + ((m - 1) * col_stride + n) * 32;
  const uintptr_t o0 = (uintptr_t)d_out, o1 = o0 + m * en * 32;
  if (s0 < o1 && o0 < s1) return H2_EINVAL;
  if (ext_log_n == 0) {            // one coefficient, one point: out[c][0] = in[c][0]
    H2_TRY(hipMemcpy2DAsync(d_out, 32, d_coeff, col_stride * 32, 32, m, hipMemcpyDeviceToDevice, k.stream));
    return H2_OK;
  }
  return coeff_to_extended_enqueue(*k.c, (int)curve, d_coeff, col_stride, log_n, m, zeta, ext_omega, ext_log_n, d_out, k.stream);
}

int h2_extended_to_coeff_device(h2_curve_t curve, const void* d_ext, uint32_t ext_log_n, size_t m, const uint64_t ext_omega_inv[4],
                                const uint64_t scale[4], const uint64_t zeta_inv[4], const void* d_t, size_t t_period, void* d_out,
                                size_t out_len, size_t out_stride, void* stream_) {
  Call k(stream_);
  if (k.rc != H2_OK) return k.rc;
  if (!curve_ok((int)curve) || ext_log_n > 30 || m > 65535) return H2_EINVAL;                  // grid.y = column
  const size_t en = (size_t)1 << ext_log_n;
  if (out_len > en || out_stride < out_len || out_stride > ((size_t)1 << 40)) return H2_EINVAL;
  if (d_t && (t_period == 0 || (t_period & (t_period - 1)) || t_period > en)) return H2_EINVAL;
  if ((((uintptr_t)d_ext | (uintptr_t)d_out | (uintptr_t)d_t) & 15) != 0) return H2_EINVAL;
  if (m == 0 || out_len == 0) return H2_OK;
  if (!d_ext || !d_out || !ext_omega_inv || !scale || !zeta_inv) return H2_EINVAL;
  // [first byte, last byte) of what is read and of what is written
  const uintptr_t s0 = (uintptr_t)d_ext, s1 = s0 + m * en * 32;
  const uintptr_t o0 = (uintptr_t)d_out, o1 = o0 + ((m - 1) * out_stride + out_len) * 32;
  if (s0 < o1 && o0 < s1) return H2_EINVAL;
  return extended_to_coeff_enqueue(*k.c, (int)curve, d_ext, ext_log_n, m, ext_omega_inv, scale, zeta_inv, d_t, t_period, d_out,
                                   out_len, out_stride, k.stream);
}

int h2_poly_scale_device(h2_curve_t curve, void* d_a, size_t n, size_t m, const uint64_t c[4], void* stream_) {
  Call k(stream_);
  if (k.rc != H2_OK) return k.rc;
  if (!curve_ok((int)curve) || !d_a || !c) return H2_EINVAL;
  if (n * m == 0) return H2_OK;
  return launched(ops_of((int)curve)->poly_scale(d_a, n * m, c, k.stream), "poly_scale_kernel");
}

int h2_poly_coset_device(h2_curve_t curve, void* d_a, size_t n, size_t m, const uint64_t g[4], void* stream_) {
  Call k(stream_);
  if (k.rc != H2_OK) return k.rc;
  if (!curve_ok((int)curve) || !d_a || !g) return H2_EINVAL;
  if (n * m == 0) return H2_OK;
  return launched(ops_of((int)curve)->poly_powers(d_a, n, m, g, k.stream), "poly_powers_kernel");
}

int h2_poly_mul_periodic_device(h2_curve_t curve, void* d_a, size_t n, size_t m, const void* d_t, size_t period,
                                void* stream_) {
  Call k(stream_);
  if (k.rc != H2_OK) return k.rc;
  if (!curve_ok((int)curve) || !d_a || !d_t || period == 0 || (period & (period - 1))) return H2_EINVAL;
  if (n * m == 0) return H2_OK;
  return launched(ops_of((int)curve)->poly_mul_periodic(d_a, n * m, d_t, period, k.stream), "poly_mul_periodic_kernel");
}

int h2_poly_inverse_device(h2_curve_t curve, void* d_a, size_t n, void* stream_) {
  Call k(stream_);
  if (k.rc != H2_OK) return k.rc;
  if (!curve_ok((int)curve) || !d_a) return H2_EINVAL;
  if (n == 0) return H2_OK;
  return launched(ops_of((int)curve)->poly_inverse(d_a, n, k.stream), "poly_inverse_kernel");
}

int h2_poly_divide_linear_device(h2_curve_t curve, const void* d_a, size_t n, const uint64_t z[4], void* d_q,
                                 void* stream_) {
  Call k(stream_);
  if (k.rc != H2_OK) return k.rc;
  if (!curve_ok((int)curve) || !d_a || !d_q || !z || d_a == d_q) return H2_EINVAL;
  if (n == 0) return H2_OK;
  ArenaLease A(k.c->div_ws, SCAN_WS_BYTES, k.stream);
  if (A.rc != H2_OK) return A.rc;
  if (int rc = launched(ops_of((int)curve)->poly_scan(0, &d_a, &d_q, z, 1, n, A.a.p, k.stream), "poly_scan kernels"); rc != H2_OK) return rc;
  return A.release();
}

int h2_poly_prefix_product_device(h2_curve_t curve, const void* d_a, size_t n, void* d_out, void* stream_) {
  Call k(stream_);
  if (k.rc != H2_OK) return k.rc;
  if (!curve_ok((int)curve) || !d_a || !d_out) return H2_EINVAL;
  if (n == 0) return H2_OK;
  ArenaLease A(k.c->div_ws, SCAN_WS_BYTES, k.stream);
  if (A.rc != H2_OK) return A.rc;
  if (int rc = launched(ops_of((int)curve)->poly_scan(1, &d_a, &d_out, nullptr, 1, n, A.a.p, k.stream), "poly_scan kernels"); rc != H2_OK) return rc;
  return A.release();
}

int h2_poly_eval_tile(void) { return POLY_EVAL_TILE; }

int h2_poly_eval_device(h2_curve_t curve, const void* const* d_polys, size_t n, const uint64_t* points, size_t q, void* d_out,
                        void* stream_) {
  Call k(stream_);
  if (k.rc != H2_OK) return k.rc;
  if (!curve_ok((int)curve) || n > POLY_EVAL_MAX_N) return H2_EINVAL;
  if (q == 0) return H2_OK;
  if (!d_polys || !points || !d_out) return H2_EINVAL;
  if (n == 0) {
    H2_TRY(hipMemsetAsync(d_out, 0, q * 32, k.stream));
    return H2_OK;
  }
  for (size_t t = 0; t < q; t++)
    if (!d_polys[t] || ((uintptr_t)d_polys[t] & 15)) return H2_EINVAL;
  return poly_eval_enqueue(*k.c, (int)curve, d_polys, n, points, q, d_out, k.stream);
}

int h2_poly_eval(h2_curve_t curve, const uint64_t* coeffs, size_t n, const uint64_t point[4], uint64_t out[4]) {
  Call k(nullptr);
  if (k.rc != H2_OK) return k.rc;
  if (!curve_ok((int)curve) || n > POLY_EVAL_MAX_N || !point || !out || (n > 0 && !coeffs)) return H2_EINVAL;
  if (n == 0) {
    memset(out, 0, 32);
    return H2_OK;
  }
  DevCtx& c = *k.c;
  const size_t off_res = h2_align256(n * 32);
  ArenaLease stage(c.stage, off_res + 32, c.stream);
  if (stage.rc != H2_OK) return stage.rc;
  char* base = (char*)c.stage.p;
  H2_TRY(hipMemcpyAsync(base, coeffs, n * 32, hipMemcpyHostToDevice, c.stream));
  const void* poly = base;
  if (int rc = poly_eval_enqueue(c, (int)curve, &poly, n, point, 1, base + off_res, c.stream); rc != H2_OK) return rc;
  H2_TRY(hipMemcpyAsync(out, base + off_res, 32, hipMemcpyDeviceToHost, c.stream));
  return stage.wait();
}

// ---- linear combinations of resident columns with linear factors divided out (h2_poly.hpp) -----------------------------
int h2_poly_lincomb_max_rounds(void) { return POLY_LINCOMB_MAX_ROUNDS; }

static_assert(sizeof(h2_lincomb_term_t) == sizeof(LincombTerm) && sizeof(h2_lincomb_job_t) == sizeof(LincombJob) &&
                  offsetof(h2_lincomb_term_t, coeff) == offsetof(LincombTerm, coeff) &&
                  offsetof(h2_lincomb_job_t, first_term) == offsetof(LincombJob, first_term),
              "the kernels read the C ABI's tables as they are");

// The overlaps h2_poly_lincomb_device rules out, every column n * 32 bytes long: an output against another job's output,
// against another job's source, and against its own job's sources (an exact alias allowed when the job divides nothing)
static bool lincomb_overlaps(const h2_lincomb_job_t* jobs, size_t n_jobs, const h2_lincomb_term_t* terms, size_t n) {
  const uintptr_t len = (uintptr_t)n * 32;
  std::vector<std::pair<uintptr_t, size_t>> src, out;      // (first byte, job)
  for (size_t j = 0; j < n_jobs; j++) {
    out.emplace_back((uintptr_t)jobs[j].d_out, j);
    for (uint32_t t = 0; t < jobs[j].n_terms; t++) src.emplace_back((uintptr_t)terms[jobs[j].first_term + t].d_poly, j);
  }
  std::sort(out.begin(), out.end());
  for (size_t a = 1; a < out.size(); a++)
    if (out[a].first - out[a - 1].first < len) return true;
  std::sort(src.begin(), src.end());
  src.erase(std::unique(src.begin(), src.end()), src.end());
  for (const auto& o : out) {
    // sources that start in (o - len, o + len)
    auto it = std::lower_bound(src.begin(), src.end(), std::make_pair(o.first >= len ? o.first - len + 1 : (uintptr_t)0, (size_t)0));
    for (; it != src.end() && it->first < o.first + len; ++it) {
      if (it->second != o.second) return true;
      if (jobs[o.second].n_points > 0 || it->first != o.first) return true;
    }
  }
  return false;
}

int h2_poly_lincomb_device(h2_curve_t curve, const h2_lincomb_job_t* jobs, size_t n_jobs, const h2_lincomb_term_t* terms,
                           size_t n_terms, const uint64_t* low, size_t n_low, const uint64_t* points, size_t n_points, size_t n,
                           void* stream_) {
  Call k(stream_);
  if (k.rc != H2_OK) return k.rc;
  if (!curve_ok((int)curve) || n > POLY_LINCOMB_MAX_N) return H2_EINVAL;
  if (n_jobs == 0) return H2_OK;
  if (!jobs || n_jobs > ((size_t)1 << 31) || n_terms > ((size_t)1 << 31) || n_low > ((size_t)1 << 31)) return H2_EINVAL;
  size_t dividing = 0;
  for (size_t j = 0; j < n_jobs; j++) {
    const h2_lincomb_job_t& J = jobs[j];
    if ((uint64_t)J.first_term + J.n_terms > n_terms || (uint64_t)J.first_low + J.n_low > n_low ||
        (uint64_t)J.first_point + J.n_points > n_points)
      return H2_EINVAL;
    if (J.n_low > n || J.n_points > (uint32_t)POLY_LINCOMB_MAX_ROUNDS) return H2_EINVAL;
    if ((J.n_terms && !terms) || (J.n_low && !low) || (J.n_points && !points)) return H2_EINVAL;
    if (!J.d_out || ((uintptr_t)J.d_out & 15)) return H2_EINVAL;
    for (uint32_t t = 0; t < J.n_terms; t++) {
      const void* p = terms[J.first_term + t].d_poly;
      if (!p || ((uintptr_t)p & 15)) return H2_EINVAL;
    }
    dividing += J.n_points > 0;
  }
  if (n == 0) return H2_OK;
  if (lincomb_overlaps(jobs, n_jobs, terms, n)) return H2_EINVAL;

  // A group is a run of consecutive jobs: at most 65535 (grid.y), and as many dividing jobs as keep their intermediate
  // columns under POLY_LINCOMB_WS_CAP (always at least one).  The groups share the scratch: the stream runs them in order
  const size_t col_bytes = h2_align256(n * 32);
  const size_t cols_cap = std::min(std::max<size_t>(1, POLY_LINCOMB_WS_CAP / col_bytes), std::max<size_t>(1, dividing));
  const size_t off_terms = h2_align256(n_jobs * sizeof(LincombJob));
  const size_t off_low = off_terms + h2_align256(n_terms * sizeof(LincombTerm));
  const size_t off_cols = off_low + h2_align256(n_low * 32);
  const size_t off_scan = off_cols + (dividing ? cols_cap * col_bytes : 0);
  ArenaLease A(k.c->div_ws, off_scan + (dividing ? SCAN_MAX_JOBS * SCAN_WS_BYTES : 0), k.stream);
  if (A.rc != H2_OK) return A.rc;
  char* base = (char*)A.a.p;

  // the tables in one upload; a job's entry names the first column it writes: d_out, or its intermediate column when an
  // odd number of divisions follows (kate_division is out of place: the rounds alternate, the last one lands in d_out)
  std::vector<char> host(off_cols, 0);
  LincombJob* hj = (LincombJob*)host.data();
  std::vector<void*> scratch_of(n_jobs, nullptr);
  std::vector<size_t> group_end;
  for (size_t j = 0, g0 = 0, used = 0; j < n_jobs; j++) {
    const bool div = jobs[j].n_points > 0;
    if (j - g0 == 65535 || (div && used == cols_cap)) {
      group_end.push_back(j);
      g0 = j;
      used = 0;
    }
    memcpy(&hj[j], &jobs[j], sizeof(LincombJob));
    if (div) {
      scratch_of[j] = base + off_cols + used++ * col_bytes;
      if (jobs[j].n_points & 1) hj[j].out = scratch_of[j];
    }
  }
  group_end.push_back(n_jobs);
  if (n_terms) memcpy(host.data() + off_terms, terms, n_terms * sizeof(LincombTerm));
  if (n_low) memcpy(host.data() + off_low, low, n_low * 32);
  // a pageable source: the runtime has read `host` when the call returns (it stages the bytes or waits for the copy)
  H2_TRY(hipMemcpyAsync(base, host.data(), off_cols, hipMemcpyHostToDevice, k.stream));

  const CurveOps* ops = ops_of((int)curve);
  for (size_t g = 0, j0 = 0; g < group_end.size(); j0 = group_end[g++]) {
    const size_t j1 = group_end[g];
    if (int rc = launched(ops->poly_lincomb((const LincombJob*)base + j0, (uint32_t)(j1 - j0), (const LincombTerm*)(base + off_terms),
                                            base + off_low, n, k.stream),
                          "poly_lincomb_kernel");
        rc != H2_OK)
      return rc;
    // round r of every job that divides by more than r points, SCAN_MAX_JOBS side by side
    for (uint32_t r = 0; r < (uint32_t)POLY_LINCOMB_MAX_ROUNDS; r++) {
      const void* src[SCAN_MAX_JOBS];
      void* dst[SCAN_MAX_JOBS];
      uint64_t z[4 * SCAN_MAX_JOBS];
      uint32_t cnt = 0;
      bool any = false;
      auto flush = [&]() -> int {
        if (cnt == 0) return H2_OK;
        const int rc = launched(ops->poly_scan(0, src, dst, z, cnt, n, base + off_scan, k.stream), "poly_scan kernels");
        cnt = 0;
        return rc;
      };
      for (size_t j = j0; j < j1; j++) {
        const uint32_t P = jobs[j].n_points;
        if (P <= r) continue;
        any = true;
        // the column before round r and the one after it: d_out when an even number of rounds is still to come
        src[cnt] = ((P - r) & 1) ? scratch_of[j] : jobs[j].d_out;
        dst[cnt] = ((P - r - 1) & 1) ? scratch_of[j] : jobs[j].d_out;
        memcpy(z + 4 * cnt, points + 4 * ((size_t)jobs[j].first_point + r), 32);
        if (++cnt == SCAN_MAX_JOBS)
          if (int rc = flush(); rc != H2_OK) return rc;
      }
      if (int rc = flush(); rc != H2_OK) return rc;
      if (!any) break;
    }
  }
  return A.release();
}

// ---- the lookup argument's permute and product steps (h2_lookup.hpp) ------------------------------------------------
int h2_lookup_tile(void) { return (int)LOOKUP_TILE; }

// [first byte, one past the last byte) of m columns of `rows` elements of `elem` bytes, stride elements apart
static std::pair<uintptr_t, uintptr_t> lookup_range(const void* p, size_t rows, size_t stride, size_t m, size_t elem = 32) {
  const uintptr_t lo = (uintptr_t)p;
  if (rows == 0) return {lo, lo};
  return {lo, lo + ((m - 1) * stride + rows) * elem};
}
static bool lookup_overlap(const std::pair<uintptr_t, uintptr_t>& a, const std::pair<uintptr_t, uintptr_t>& b) {
  return a.first < b.second && b.first < a.second && a.first != a.second && b.first != b.second;
}

int h2_lookup_permute_device(h2_curve_t curve, const void* d_input, const void* d_table, size_t usable_rows, size_t col_stride,
                             size_t m, void* d_permuted_input, void* d_permuted_table, void* d_status, void* stream_) {
  Call k(stream_);
  if (k.rc != H2_OK) return k.rc;
  const size_t u = usable_rows;
  if (!curve_ok((int)curve) || u > LOOKUP_MAX_ROWS || col_stride < u || (col_stride && m > LOOKUP_MAX_CELLS / col_stride)) return H2_EINVAL;
  if ((((uintptr_t)d_input | (uintptr_t)d_table | (uintptr_t)d_permuted_input | (uintptr_t)d_permuted_table) & 15) || ((uintptr_t)d_status & 3))
    return H2_EINVAL;
  if (m == 0) return H2_OK;
  if (!d_status || (u > 0 && (!d_input || !d_table || !d_permuted_input || !d_permuted_table))) return H2_EINVAL;
  const auto in = lookup_range(d_input, u, col_stride, m), tab = lookup_range(d_table, u, col_stride, m);
  const auto pin = lookup_range(d_permuted_input, u, col_stride, m), ptab = lookup_range(d_permuted_table, u, col_stride, m);
  const auto st = lookup_range(d_status, 1, 1, m, 4);
  for (const auto* out : {&pin, &ptab, &st})
    if (lookup_overlap(*out, in) || lookup_overlap(*out, tab)) return H2_EINVAL;
  if (lookup_overlap(pin, ptab) || lookup_overlap(pin, st) || lookup_overlap(ptab, st)) return H2_EINVAL;
  // the groups' bounds are proven before the first of them is enqueued
  const size_t group = u ? lookup_group(u, m) : m;
  for (size_t j0 = 0; u && j0 < m; j0 += group) {
    const size_t mm = std::min(group, m - j0);
    const LookupWorkspace ws = lookup_workspace(u, mm);
    if (const char* broken = lookup_check(ws, u, mm, col_stride, ws.total)) {
      g_h2.last_error = std::string("lookup launch geometry: ") + broken;
      return H2_EDEVICE;
    }
  }
  H2_TRY(hipMemsetAsync(d_status, 0, 4 * m, k.stream));
  if (u == 0) return H2_OK;
  const CurveOps* ops = ops_of((int)curve);
  for (size_t j0 = 0; j0 < m; j0 += group) {             // the groups share the workspace: the stream runs them in order
    const size_t mm = std::min(group, m - j0);
    const LookupWorkspace ws = lookup_workspace(u, mm);
    ArenaLease A(k.c->msm_ws.of(k.stream), ws.total, k.stream);      // the MSM workspace, idle here
    if (A.rc != H2_OK) return A.rc;
    if (const char* broken = lookup_check(ws, u, mm, col_stride, A.a.bytes)) {      // the arena the lease handed out must hold the layout
      g_h2.last_error = std::string("lookup launch geometry: ") + broken;
      return H2_EDEVICE;
    }
    const size_t skip = j0 * col_stride * 32;
    if (int rc = launched(ops->lookup_permute((const char*)d_input + skip, (const char*)d_table + skip, col_stride, ws, (char*)A.a.p,
                                              (char*)d_permuted_input + skip, (char*)d_permuted_table + skip, (uint32_t*)d_status + j0,
                                              k.stream),
                          "lookup permute kernels");
        rc != H2_OK)
      return rc;
    if (int rc = A.release(); rc != H2_OK) return rc;
  }
  return H2_OK;
}

int h2_lookup_product_device(h2_curve_t curve, const void* d_input, const void* d_table, const void* d_permuted_input,
                             const void* d_permuted_table, size_t usable_rows, size_t col_stride, size_t m, const uint64_t beta[4],
                             const uint64_t gamma[4], void* d_z, void* stream_) {
  Call k(stream_);
  if (k.rc != H2_OK) return k.rc;
  const size_t u = usable_rows;
  if (!curve_ok((int)curve) || u > LOOKUP_MAX_ROWS || col_stride < u + 1 || m > LOOKUP_MAX_CELLS / col_stride) return H2_EINVAL;
  if (((uintptr_t)d_input | (uintptr_t)d_table | (uintptr_t)d_permuted_input | (uintptr_t)d_permuted_table | (uintptr_t)d_z) & 15) return H2_EINVAL;
  if (m == 0) return H2_OK;
  if (!d_z || !beta || !gamma || (u > 0 && (!d_input || !d_table || !d_permuted_input || !d_permuted_table))) return H2_EINVAL;
  const auto z = lookup_range(d_z, u + 1, col_stride, m);
  for (const void* src : {d_input, d_table, d_permuted_input, d_permuted_table})
    if (lookup_overlap(z, lookup_range(src, u, col_stride, m))) return H2_EINVAL;
  const CurveOps* ops = ops_of((int)curve);
  for (size_t j0 = 0; j0 < m; j0 += 65535) {             // grid.y = column
    const size_t skip = j0 * col_stride * 32;
    if (int rc = launched(ops->lookup_ratio((const char*)d_input + skip, (const char*)d_table + skip, (const char*)d_permuted_input + skip,
                                            (const char*)d_permuted_table + skip, u, col_stride, std::min<size_t>(65535, m - j0), beta,
                                            gamma, (char*)d_z + skip, k.stream),
                          "lookup_ratio_kernel");
        rc != H2_OK)
      return rc;
  }
  // z[i] = prod_{t < i} ratio[t] over u + 1 rows, in place, SCAN_MAX_JOBS columns side by side
  ArenaLease A(k.c->div_ws, SCAN_MAX_JOBS * SCAN_WS_BYTES, k.stream);
  if (A.rc != H2_OK) return A.rc;
  for (size_t j0 = 0; j0 < m; j0 += SCAN_MAX_JOBS) {     // the groups share the scratch: the stream runs them in order
    const uint32_t cnt = (uint32_t)std::min<size_t>(SCAN_MAX_JOBS, m - j0);
    const void* src[SCAN_MAX_JOBS];
    void* dst[SCAN_MAX_JOBS];
    for (uint32_t j = 0; j < cnt; j++) src[j] = dst[j] = (char*)d_z + (j0 + j) * col_stride * 32;
    if (int rc = launched(ops->poly_scan(1, src, dst, nullptr, cnt, u + 1, A.a.p, k.stream), "poly_scan kernels"); rc != H2_OK) return rc;
  }
  return A.release();
}

// ---- the permutation argument's grand products, chained on the device (h2_permutation.hpp) ---------------------------
int h2_permutation_tile(void) { return (int)perm_tile(); }

int h2_permutation_product_device(h2_curve_t curve, const void* const* d_values, const void* const* d_sigma, size_t n_cols, size_t chunk_len,
                                  size_t usable_rows, size_t m, const uint64_t* beta, const uint64_t* gamma, const uint64_t omega[4],
                                  const uint64_t delta[4], void* d_z, size_t col_stride, void* stream_) {
  Call k(stream_);
  if (k.rc != H2_OK) return k.rc;
  const size_t u = usable_rows;
  if (!curve_ok((int)curve) || (chunk_len == 0 && n_cols > 0) || u > PERM_MAX_ROWS || col_stride < u + 1) return H2_EINVAL;
  const size_t S = n_cols ? (n_cols - 1) / chunk_len + 1 : 0;
  if (S && m && (m > PERM_MAX_CELLS / S || m * S > PERM_MAX_CELLS / col_stride)) return H2_EINVAL;
  if (m == 0 || n_cols == 0) return H2_OK;
  if (!d_values || !d_sigma || !beta || !gamma || !omega || !delta || !d_z || ((uintptr_t)d_z & 15)) return H2_EINVAL;
  // the tables are m n_cols entries of host and device memory: bounded before anything is sized by them
  if (n_cols > ((size_t)1 << 31) || m > ((size_t)1 << 32) / n_cols) {
    g_h2.last_error = "permutation launch geometry: m n_cols <= 2^32";
    return H2_EDEVICE;
  }
  if (u > 0) {
    const auto z = lookup_range(d_z, u + 1, col_stride, m * S);
    for (size_t t = 0; t < m * n_cols + n_cols; t++) {
      const void* src = t < m * n_cols ? d_values[t] : d_sigma[t - m * n_cols];
      if (!src || ((uintptr_t)src & 15) || lookup_overlap(z, lookup_range(src, u, u, 1))) return H2_EINVAL;
    }
  }
  return permutation_product_enqueue(*k.c, (int)curve, d_values, d_sigma, n_cols, chunk_len, u, m, beta, gamma, omega, delta, d_z, col_stride,
                                     k.stream);
}

// ---- expressions over resident columns --------------------------------------------------------------------------------
int h2_expr_compile(h2_curve_t curve, const h2_expr_node_t* nodes, size_t n_nodes, const uint64_t* consts, size_t n_consts,
                    uint32_t n_cols, uint32_t n_vars, uint64_t* handle_out) {
  std::lock_guard<std::recursive_mutex> lk(g_h2_mu);
  auto refuse = [](const char* rule) {
    g_h2.last_error = std::string("expr: ") + rule;
    return (int)H2_EINVAL;
  };
  if (!curve_ok((int)curve)) return refuse("unknown curve");
  if (!handle_out || !nodes || (n_consts && !consts)) return refuse("null pointer");
  if (n_nodes == 0 || n_nodes > EXPR_MAX_COUNT) return refuse("n_nodes must be 1 .. 2^20");
  if (n_consts > EXPR_MAX_COUNT || n_vars > EXPR_MAX_COUNT) return refuse("n_consts and n_vars may be at most 2^20");
  if (n_cols > (1u << 22)) return refuse("n_cols may be at most 2^22");
  ExprEntry e{};
  e.curve = (int)curve;
  try {
    H2_BY_SCALAR_FIELD((int)curve, expr_compile_t)(nodes, n_nodes, consts, n_consts, n_cols, n_vars, e);
  } catch (const product::Fail& f) {
    g_h2.last_error = f.what;
    return f.status;
  } catch (const std::exception& x) {
    g_h2.last_error = x.what();
    return H2_ENOMEM;
  }
  e.info.curve = (uint32_t)curve;
  const uint64_t h = g_h2.next_handle++;
  g_h2.exprs[h] = std::move(e);
  *handle_out = h;
  return H2_OK;
}

int h2_expr_release(uint64_t handle) {
  std::lock_guard<std::recursive_mutex> lk(g_h2_mu);
  auto it = g_h2.exprs.find(handle);
  if (it == g_h2.exprs.end()) return H2_EHANDLE;
  for (size_t i = 0; i < it->second.d_code.size() && i < g_h2.ctx.size(); i++) {
    if (!it->second.d_code[i]) continue;
    DeviceGuard dg(g_h2.ctx[i].device);
    (void)hipDeviceSynchronize();     // launches on caller streams may still read the code
    (void)hipFree(it->second.d_code[i]);
  }
  g_h2.exprs.erase(it);
  return H2_OK;
}

int h2_expr_info(uint64_t handle, h2_expr_info_t* out) {
  std::lock_guard<std::recursive_mutex> lk(g_h2_mu);
  if (!out) return H2_EINVAL;
  auto it = g_h2.exprs.find(handle);
  if (it == g_h2.exprs.end()) return H2_EHANDLE;
  *out = it->second.info;
  return H2_OK;
}

int h2_expr_dump(uint64_t handle, uint8_t* out, size_t cap, size_t* out_len) {
  std::lock_guard<std::recursive_mutex> lk(g_h2_mu);
  auto it = g_h2.exprs.find(handle);
  if (it == g_h2.exprs.end()) return H2_EHANDLE;
  const std::vector<uint8_t>& d = it->second.dump;
  if (out_len) *out_len = d.size();
  if (!out || cap < d.size()) return H2_EINVAL;       // *out_len says how much is needed
  memcpy(out, d.data(), d.size());
  return H2_OK;
}

int h2_expr_eval_device(uint64_t handle, const void* const* d_cols, const uint32_t* log_len, const uint64_t* vars, size_t m,
                        uint32_t log_rows, uint32_t rot_step, void* d_out, size_t out_stride, void* stream_) {
  Call k(stream_);
  if (k.rc != H2_OK) return k.rc;
  auto it = g_h2.exprs.find(handle);
  if (it == g_h2.exprs.end()) return H2_EHANDLE;
  ExprEntry& e = it->second;
  const size_t n_cols = e.info.n_cols, n_vars = e.info.n_vars, nconsts = e.table.size() / 4;
  if (log_rows > 28 || m > EXPR_MAX_INSTANCES) return H2_EINVAL;
  const size_t rows = (size_t)1 << log_rows;
  if (out_stride < rows || (m && out_stride > ((size_t)1 << 57) / m)) return H2_EINVAL;
  if (m == 0) return H2_OK;
  if (!d_out || ((uintptr_t)d_out & 15) || (n_cols && (!d_cols || !log_len)) || (n_vars && !vars)) return H2_EINVAL;
  for (size_t c = 0; c < n_cols; c++)
    if (log_len[c] > log_rows) return H2_EINVAL;
  // every column's bytes against the rows that are written: [0, rows) of each instance's window of out_stride rows.  A
  // column inside [d_out, the last written byte) starts in the window of one instance: it may neither start before that
  // instance's last written row nor reach the next instance's first
  const uintptr_t o0 = (uintptr_t)d_out, window = out_stride * 32, written = rows * 32, o1 = o0 + (m - 1) * window + written;
  for (size_t p = 0; p < m; p++)
    for (size_t c = 0; c < n_cols; c++) {
      const uintptr_t s0 = (uintptr_t)d_cols[p * n_cols + c], s1 = s0 + ((uintptr_t)32 << log_len[c]);
      if (!s0 || (s0 & 15)) return H2_EINVAL;
      if (s0 < o1 && o0 < s1) {
        const uintptr_t q = s0 > o0 ? (s0 - o0) / window : 0, w0 = o0 + q * window;
        if (s0 < w0 + written || (q + 1 < m && s1 > w0 + window)) return H2_EINVAL;
      }
    }
  for (size_t t = 0; t < m * n_vars; t++)
    if (!H2_BY_SCALAR_FIELD(e.curve, mont_canonical)(vars + 4 * t)) return H2_EINVAL;
  DevCtx& c = *k.c;
  const size_t ci = ctx_index(&c);
  // instances per launch: grid.y, and what keeps the group's constant tables under EXPR_TABLE_CAP
  const size_t group = std::min<size_t>({m, (size_t)65535, std::max<size_t>(1, EXPR_TABLE_CAP / (nconsts * 32))});
  // the host side of the tables (up to EXPR_TABLE_CAP) before anything is enqueued: nothing may throw across the C ABI
  std::vector<uint32_t> masks;
  std::vector<uint64_t> tables;
  try {
    masks.resize(n_cols);
    tables.resize(group * nconsts * 4);
    if (e.d_code.size() != g_h2.ctx.size()) e.d_code.assign(g_h2.ctx.size(), nullptr);
  } catch (const std::bad_alloc&) {
    g_h2.last_error = "expr: no host memory for the instances' constant tables";
    return H2_ENOMEM;
  }
  if (!e.d_code[ci]) {
    // uploaded on the library's stream and finished before anybody uses it: later calls bring any stream (once per context)
    void* p = nullptr;
    if (int rc = device_alloc(&p, e.code.size() * 4, "expr code"); rc != H2_OK) return rc;
    DeviceBuffer owner(p);
    H2_TRY(hipMemcpyAsync(p, e.code.data(), e.code.size() * 4, hipMemcpyHostToDevice, c.stream));
    H2_TRY(hipStreamSynchronize(c.stream));
    e.d_code[ci] = owner.release();
  }
  const size_t mask_bytes = h2_align256(n_cols * 4 + 4), ptr_bytes = h2_align256(group * n_cols * sizeof(void*) + 8);
  ArenaLease A(c.div_ws, mask_bytes + ptr_bytes + group * nconsts * 32, k.stream);
  if (A.rc != H2_OK) return A.rc;
  uint32_t* d_masks = (uint32_t*)A.a.p;
  const void** d_ptrs = (const void**)((char*)A.a.p + mask_bytes);
  void* d_tables = (char*)A.a.p + mask_bytes + ptr_bytes;
  // pageable sources: the runtime has read them when each call returns (it stages the bytes or waits for the copy)
  for (size_t j = 0; j < n_cols; j++) masks[j] = (1u << log_len[j]) - 1;
  if (n_cols) H2_TRY(hipMemcpyAsync(d_masks, masks.data(), n_cols * 4, hipMemcpyHostToDevice, k.stream));
  const CurveOps* ops = ops_of(e.curve);
  for (size_t p0 = 0; p0 < m; p0 += group) {             // the groups share the scratch: the stream runs them in order
    const size_t cnt = std::min(group, m - p0);
    H2_BY_SCALAR_FIELD(e.curve, expr_fill_tables)(e, vars, p0, cnt, tables.data());
    if (n_cols) H2_TRY(hipMemcpyAsync(d_ptrs, d_cols + p0 * n_cols, cnt * n_cols * sizeof(void*), hipMemcpyHostToDevice, k.stream));
    H2_TRY(hipMemcpyAsync(d_tables, tables.data(), cnt * nconsts * 32, hipMemcpyHostToDevice, k.stream));
    if (int rc = launched(ops->expr_launch(e.d_code[ci], e.info.instructions, d_ptrs, (uint32_t)n_cols, d_masks, d_tables, (uint32_t)nconsts,
                                           (char*)d_out + p0 * out_stride * 32, out_stride, rot_step, (uint32_t)rows, (uint32_t)cnt,
                                           e.info.lds_bytes, k.stream),
                          "expr_kernel");
        rc != H2_OK)
      return rc;
  }
  return A.release();
}

int h2_chacha20_scalars_device(h2_curve_t curve, const uint8_t seed[32], uint64_t first_block, size_t n, void* d_out,
                               void* stream_) {
  Call k(stream_);
  if (k.rc != H2_OK) return k.rc;
  if (!curve_ok((int)curve) || !seed || !d_out) return H2_EINVAL;
  if (n == 0) return H2_OK;
  uint32_t key[8];
  for (int i = 0; i < 8; i++)
    key[i] = (uint32_t)seed[4 * i] | ((uint32_t)seed[4 * i + 1] << 8) | ((uint32_t)seed[4 * i + 2] << 16) |
             ((uint32_t)seed[4 * i + 3] << 24);
  return launched(ops_of((int)curve)->chacha20_scalars(d_out, n, first_block, key, k.stream), "chacha20_scalars_kernel");
}

// ---- the inner product argument on a registered table (h2_ipa.hpp) ---------------------------------------------------
static_assert(H2_IPA_MAX_K == IPA_MAX_K, "the header states the kernels' maximum");
static bool ipa_dev_ptr(const void* p) { return p && !((uintptr_t)p & 15); }

int h2_ipa_challenge_products_device(h2_curve_t curve, const uint64_t* u, uint32_t k_, const uint64_t init[4], void* d_out,
                                     void* stream_) {
  Call k(stream_);
  if (k.rc != H2_OK) return k.rc;
  if (!curve_ok((int)curve) || k_ == 0 || k_ > IPA_MAX_K || !u || !init || !ipa_dev_ptr(d_out)) return H2_EINVAL;
  return launched(ops_of((int)curve)->ipa_s_products(u, k_, init, d_out, k.stream), "ipa_s_kernel");
}

// the sum kernel over `count` rows of a table that is in HBM already (ipa_sum_fill's layout), in launches of IPA_SUM_GROUP
// rows, the first one overwriting d_out unless `accumulate`: h2_ipa_challenge_products_sum_device's launch and the batch
// verifier's, whose table the prepare kernel wrote
static int ipa_sum_run(const CurveOps* ops, const void* d_table, size_t count, uint32_t k, void* d_out, bool accumulate, hipStream_t stream) {
  const size_t row = ipa_sum_stride(k);
  for (size_t p0 = 0; p0 < count; p0 += IPA_SUM_GROUP) {
    const size_t cnt = std::min(IPA_SUM_GROUP, count - p0);
    if (int rc = launched(ops->ipa_s_sum((const char*)d_table + p0 * row * 4, (uint32_t)cnt, k, d_out, accumulate || p0 > 0, stream),
                          "ipa_s_sum_kernel");
        rc != H2_OK)
      return rc;
  }
  return H2_OK;
}

int h2_ipa_challenge_products_sum_device(h2_curve_t curve, const uint64_t* u, const uint64_t* init, uint32_t k_, size_t count,
                                         void* d_out, void* stream_) {
  Call k(stream_);
  if (k.rc != H2_OK) return k.rc;
  if (!curve_ok((int)curve) || k_ == 0 || k_ > IPA_MAX_K || !ipa_dev_ptr(d_out) || (count && (!u || !init))) return H2_EINVAL;
  const size_t n = (size_t)1 << k_;
  if (count == 0) {
    H2_TRY(hipMemsetAsync(d_out, 0, n * 32, k.stream));
    return H2_OK;
  }
  // the group's table in the scan arena for the length of the call; the groups share it: the stream runs them in order
  const size_t group = std::min(count, IPA_SUM_GROUP), row = ipa_sum_stride(k_);
  std::vector<int32_t> host;
  try {
    host.resize(group * row);
  } catch (const std::bad_alloc&) {
    g_h2.last_error = "ipa: no host memory for the challenge table";
    return H2_ENOMEM;
  }
  ArenaLease A(k.c->div_ws, group * row * 4, k.stream);
  if (A.rc != H2_OK) return A.rc;
  const CurveOps* ops = ops_of((int)curve);
  for (size_t p0 = 0; p0 < count; p0 += group) {
    const size_t cnt = std::min(group, count - p0);
    H2_BY_SCALAR_FIELD((int)curve, ipa_sum_fill)(u + 4 * p0 * k_, init + 4 * p0, k_, cnt, host.data());
    // a pageable source: the runtime has read `host` when the call returns (it stages the bytes or waits for the copy)
    H2_TRY(hipMemcpyAsync(A.a.p, host.data(), cnt * row * 4, hipMemcpyHostToDevice, k.stream));
    if (int rc = ipa_sum_run(ops, A.a.p, cnt, k_, d_out, p0 > 0, k.stream); rc != H2_OK) return rc;
  }
  return A.release();
}

// ---- the prover's rounds: m openings in lockstep (h2_ipa.hpp, IpaBatchLayout); the single calls are m = 1 -----------------
static_assert(H2_IPA_MAX_BATCH == IPA_MAX_BATCH, "the header states the kernels' maximum");

int h2_ipa_batch_state_bytes(uint32_t k, size_t m, size_t* out) {
  if (k == 0 || k > IPA_MAX_K || m == 0 || m > IPA_MAX_BATCH || !out) return H2_EINVAL;
  *out = IpaBatchLayout(k, m).total * 32;
  return H2_OK;
}

int h2_ipa_state_bytes(uint32_t k, size_t* out) { return h2_ipa_batch_state_bytes(k, 1, out); }

// The call's scalars: rows[r] holds m x 4 limbs (null: a row of zeros); `ptrs` (begin only) are the m device pointers.  For
// m >= 2 they become the table at the end of the state, the pointers behind row 0: one copy, enqueued before the call's
// kernels.  For m = 1 they go into `one`, which travels in the kernels' arguments, and nothing is enqueued.
static int ipa_scalars(const IpaBatchLayout& L, const uint64_t* const* rows, size_t n_rows, const void* const* ptrs, void* d_state,
                       hipStream_t stream, IpaOne& one) {
  const size_t m = L.m;
  memset(&one, 0, sizeof one);
  if (m == 1) {
    for (size_t r = 0; r < n_rows; r++)
      if (rows[r]) memcpy(one.v[r], rows[r], 32);
    if (ptrs) one.p = ptrs[0];
    return H2_OK;
  }
  uint64_t host[IPA_BATCH_SCALARS * IPA_MAX_BATCH * 4];
  for (size_t r = 0; r < n_rows; r++) {
    if (rows[r])
      memcpy(host + r * m * 4, rows[r], m * 32);
    else
      memset(host + r * m * 4, 0, m * 32);
  }
  size_t words = n_rows * m * 4;
  if (ptrs) {
    for (size_t i = 0; i < m; i++) host[words + i] = (uint64_t)(uintptr_t)ptrs[i];
    words += m;
  }
  // a pageable source: the runtime has read `host` when the call returns (it stages the bytes or waits for the copy)
  H2_TRY(hipMemcpyAsync((char*)d_state + L.scal * 32, host, words * 8, hipMemcpyHostToDevice, stream));
  return H2_OK;
}

int h2_ipa_begin_batch_device(h2_curve_t curve, uint32_t k_, size_t m, const void* const* d_p, const uint64_t* x3, void* d_state,
                              void* stream_) {
  Call k(stream_);
  if (k.rc != H2_OK) return k.rc;
  if (!curve_ok((int)curve) || k_ == 0 || k_ > IPA_MAX_K || m == 0 || m > IPA_MAX_BATCH || !d_p || !x3 || !ipa_dev_ptr(d_state))
    return H2_EINVAL;
  for (size_t i = 0; i < m; i++)
    if (!ipa_dev_ptr(d_p[i])) return H2_EINVAL;
  const IpaBatchLayout L(k_, m);
  const uint64_t* rows[1] = {x3};
  IpaOne one;
  if (int rc = ipa_scalars(L, rows, 1, d_p, d_state, k.stream, one); rc != H2_OK) return rc;
  return launched(ops_of((int)curve)->ipa_begin(k_, m, one, d_state, k.stream), "ipa_begin_kernel");
}

int h2_ipa_round_batch_device(h2_curve_t curve, uint64_t bases, uint32_t k_, uint32_t j, size_t m, void* d_state,
                              const uint64_t* u_prev, const uint64_t* u_prev_inv, const uint64_t* z, const uint64_t* l_blind,
                              const uint64_t* r_blind, void* d_out_affine, void* stream_) {
  Call k(stream_);
  if (k.rc != H2_OK) return k.rc;
  if (!curve_ok((int)curve) || k_ == 0 || k_ > IPA_MAX_K || j >= k_ || m == 0 || m > IPA_MAX_BATCH) return H2_EINVAL;
  if (!ipa_dev_ptr(d_state) || !ipa_dev_ptr(d_out_affine) || !z || !l_blind || !r_blind) return H2_EINVAL;
  if (j == 0 ? (u_prev || u_prev_inv) : (!u_prev || !u_prev_inv)) return H2_EINVAL;
  const IpaBatchLayout L(k_, m);
  const BasesEntry* be = nullptr;
  if (int rc = msm_common_checks((int)curve, bases, 0, L.col_stride, 2 * m, &be); rc != H2_OK) return rc;
  if (be->n != L.col_stride) return H2_EINVAL;          // exactly G || U || W
  // the MSM's own refusals before the table copy and the kernels in front of it: nothing is enqueued for a refused call
  if (int rc = msm_device_plan_check(*be, L.col_stride, L.col_stride, 2 * m); rc != H2_OK) return rc;
  const uint64_t* rows[IPA_BATCH_SCALARS] = {u_prev, u_prev_inv, z, l_blind, r_blind};
  IpaOne one;
  if (int rc = ipa_scalars(L, rows, IPA_BATCH_SCALARS, nullptr, d_state, k.stream, one); rc != H2_OK) return rc;
  if (int rc = launched(ops_of((int)curve)->ipa_round(k_, j, m, one, d_state, k.stream), "ipa_round_kernel"); rc != H2_OK) return rc;
  return msm_device_run(*k.c, (int)curve, *be, (const char*)d_state + L.col * 32, 0, L.col_stride, L.col_stride, 2 * m, d_out_affine,
                        true, k.stream);
}

// d_s_out: m x 2^k elements or null; only h2_ipa_final_device has an argument for it
static int ipa_final_run(h2_curve_t curve, uint32_t k_, size_t m, void* d_state, const uint64_t* u_last, const uint64_t* u_last_inv,
                         void* d_out, void* d_s_out, void* stream_) {
  Call k(stream_);
  if (k.rc != H2_OK) return k.rc;
  if (!curve_ok((int)curve) || k_ == 0 || k_ > IPA_MAX_K || m == 0 || m > IPA_MAX_BATCH || !ipa_dev_ptr(d_state) ||
      !ipa_dev_ptr(d_out) || !u_last || !u_last_inv)
    return H2_EINVAL;
  if (d_s_out && ((uintptr_t)d_s_out & 15)) return H2_EINVAL;
  const IpaBatchLayout L(k_, m);
  const uint64_t* rows[2] = {u_last, u_last_inv};
  IpaOne one;
  if (int rc = ipa_scalars(L, rows, 2, nullptr, d_state, k.stream, one); rc != H2_OK) return rc;
  return launched(ops_of((int)curve)->ipa_final(k_, m, one, d_state, d_out, d_s_out, k.stream), "ipa_final_kernel");
}

int h2_ipa_final_batch_device(h2_curve_t curve, uint32_t k_, size_t m, void* d_state, const uint64_t* u_last,
                              const uint64_t* u_last_inv, void* d_out, void* stream_) {
  return ipa_final_run(curve, k_, m, d_state, u_last, u_last_inv, d_out, nullptr, stream_);
}

// the single opening: the batch of one
int h2_ipa_begin_device(h2_curve_t curve, uint32_t k_, const void* d_p, const uint64_t x3[4], void* d_state, void* stream_) {
  return h2_ipa_begin_batch_device(curve, k_, 1, &d_p, x3, d_state, stream_);
}

int h2_ipa_round_device(h2_curve_t curve, uint64_t bases, uint32_t k_, uint32_t j, void* d_state, const uint64_t* u_prev,
                        const uint64_t* u_prev_inv, const uint64_t z[4], const uint64_t l_blind[4], const uint64_t r_blind[4],
                        void* d_out_affine, void* stream_) {
  return h2_ipa_round_batch_device(curve, bases, k_, j, 1, d_state, u_prev, u_prev_inv, z, l_blind, r_blind, d_out_affine, stream_);
}

int h2_ipa_final_device(h2_curve_t curve, uint32_t k_, void* d_state, const uint64_t u_last[4], const uint64_t u_last_inv[4],
                        void* d_out, void* d_s_out, void* stream_) {
  return ipa_final_run(curve, k_, 1, d_state, u_last, u_last_inv, d_out, d_s_out, stream_);
}

// ---- the transcript midstate (host only) ---------------------------------------------------------------------------------
static_assert(sizeof(h2_transcript_state_t) == Blake2b::STATE_BYTES && sizeof(h2_transcript_state_t) == TRANSCRIPT_STATE_BYTES,
              "the header's struct is the exported Blake2b state and the replay kernel's");

int h2_transcript_init(h2_transcript_state_t* state) {
  if (!state) return H2_EINVAL;
  Blake2b("Halo2-Transcript").export_state((uint8_t*)state);
  return H2_OK;
}

int h2_transcript_absorb(h2_transcript_state_t* state, const uint8_t* bytes, size_t len) {
  if (!state || (len && !bytes)) return H2_EINVAL;
  Blake2b b;
  if (!b.import_state((const uint8_t*)state)) return H2_EINVAL;
  b.update(bytes, len);
  b.export_state((uint8_t*)state);
  return H2_OK;
}

int h2_transcript_challenge(h2_curve_t curve, h2_transcript_state_t* state, uint64_t out[4]) {
  if (!curve_ok((int)curve) || !state || !out) return H2_EINVAL;
  Blake2b b;
  if (!b.import_state((const uint8_t*)state)) return H2_EINVAL;
  const uint8_t zero = 0;
  b.update(&zero, 1);
  uint8_t digest[64];
  b.digest(digest);                                      // of a copy: the state keeps absorbing
  b.export_state((uint8_t*)state);
  H2_BY_SCALAR_FIELD((int)curve, transcript_reduce)(digest, out);
  return H2_OK;
}

// ---- the IPA batch verifier (h2_ipa_verify.hpp) --------------------------------------------------------------------------
int h2_ipa_replay_device(h2_curve_t curve, uint32_t k_, size_t count, const void* d_states, const void* d_points,
                         const void* d_point_status, const void* d_scalars, void* d_out, void* d_status, void* d_states_out,
                         void* stream_) {
  Call k(stream_);
  if (k.rc != H2_OK) return k.rc;
  if (!curve_ok((int)curve) || !ops_of((int)curve)->ipa_replay || k_ == 0 || k_ > IPA_MAX_K || count > ((size_t)1 << 24)) return H2_EINVAL;
  if (count == 0) return H2_OK;
  if (!ipa_dev_ptr(d_states) || !ipa_dev_ptr(d_points) || !d_point_status || !ipa_dev_ptr(d_scalars) || !ipa_dev_ptr(d_out) || !d_status)
    return H2_EINVAL;
  if (d_states_out && ((uintptr_t)d_states_out & 15)) return H2_EINVAL;
  return launched(ops_of((int)curve)->ipa_replay(k_, count, d_states, d_points, d_point_status, d_scalars, d_out, d_status, d_states_out,
                                                 k.stream),
                  "ipa_replay_kernel");
}

int h2_ipa_verify_proofs(h2_curve_t curve, uint64_t bases, uint32_t k_, size_t count, const h2_transcript_state_t* states,
                         const uint8_t* const* proofs, const size_t* proof_lens, const uint64_t* commitments, const uint64_t* x3,
                         const uint64_t* v, h2_rng_fill_t rng, void* rng_ctx, int* ok, int* all_ok, size_t* checks_out) {
  Call k(nullptr);
  if (k.rc != H2_OK) return k.rc;
  if (!curve_ok((int)curve) || !ops_of((int)curve)->ipa_replay || k_ == 0 || k_ > IPA_MAX_K) return H2_EINVAL;
  if (count && (!states || !proofs || !proof_lens || !commitments || !x3 || !v || !ok)) return H2_EINVAL;
  const size_t n = (size_t)1 << k_, per = 2 * (size_t)k_ + 1, need = (per + 2) * 32;
  const BasesEntry* be = nullptr;
  if (int rc = msm_common_checks((int)curve, bases, 0, n + 2, 1, &be); rc != H2_OK) return rc;
  if (be->n != n + 2) return H2_EINVAL;                   // exactly G || U || W
  if (int rc = msm_device_plan_check(*be, n + 2, n + 2, 1); rc != H2_OK) return rc;
  if (count > ((size_t)1 << 24) || count * (per + 1) > MSM_POINTS_MAX_N) return H2_EINVAL;
  if (!H2_BY_SCALAR_FIELD((int)curve, ipa_canonical)(x3, count) || !H2_BY_SCALAR_FIELD((int)curve, ipa_canonical)(v, count))
    return H2_EINVAL;
  for (size_t i = 0; i < count; i++)
    if (states[i].buflen > 128 || (proof_lens[i] && !proofs[i])) return H2_EINVAL;
  if (all_ok) *all_ok = 1;
  if (checks_out) *checks_out = 0;
  if (count == 0) return H2_OK;
  const CurveOps* ops = ops_of((int)curve);
  hipStream_t stream = k.stream;
  try {
    // a proof of any other length is refused here: a short stream fails verify_proof's reads, trailing bytes are the caller's
    std::vector<size_t> item;                              // device proof -> item
    for (size_t i = 0; i < count; i++) {
      ok[i] = 0;
      if (proof_lens[i] == need) item.push_back(i);
    }
    if (all_ok) *all_ok = 0;
    const size_t M = item.size();
    if (M == 0) return H2_OK;
    const size_t G = M * per, row = ipa_sum_stride(k_);
    auto up16 = [](size_t x) { return (x + 15) & ~(size_t)15; };
    // the scratch: the decompression's output with the commitments behind it is the points MSM's operand, and everything the
    // host uploads -- from the commitments on -- is one range
    size_t off = 0;
    auto region = [&](size_t bytes) { const size_t o = off; off += up16(bytes); return o; };
    const size_t o_points = region(G * 64), o_commit = region(M * 64), o_wire = region(G * 32), o_states = region(M * sizeof(h2_transcript_state_t)),
                 o_scalars = region(M * 64), o_x3 = region(M * 32), o_v = region(M * 32), o_upload_end = off, o_pstatus = region(G),
                 o_replay = region(M * (k_ + 4) * 32), o_status = region(M), o_weights = region(M * IPA_WEIGHT_WORDS * 4),
                 o_scal = region((G + M) * 32), o_table = region(M * row * 4), o_terms = region(M * 96), o_col = region((n + 2) * 32),
                 o_jac = region(3 * 96);
    ArenaLease A(k.c->stage, off, stream);
    if (A.rc != H2_OK) return A.rc;
    char* base = (char*)A.a.p;
    std::vector<uint8_t> host(o_upload_end - o_commit, 0);
    for (size_t j = 0; j < M; j++) {
      const size_t i = item[j];
      memcpy(&host[o_commit - o_commit + j * 64], commitments + 8 * i, 64);
      memcpy(&host[o_wire - o_commit + j * per * 32], proofs[i], per * 32);
      memcpy(&host[o_states - o_commit + j * sizeof(h2_transcript_state_t)], &states[i], sizeof(h2_transcript_state_t));
      memcpy(&host[o_scalars - o_commit + j * 64], proofs[i] + per * 32, 64);
      memcpy(&host[o_x3 - o_commit + j * 32], x3 + 4 * i, 32);
      memcpy(&host[o_v - o_commit + j * 32], v + 4 * i, 32);
    }
    // a pageable source: the runtime has read `host` when the call returns (it stages the bytes or waits for the copy)
    H2_TRY(hipMemcpyAsync(base + o_commit, host.data(), host.size(), hipMemcpyHostToDevice, stream));
    if (int rc = launched(ops->pasta_points_decompress(base + o_wire, base + o_points, base + o_pstatus, (uint32_t)G, stream),
                          "points_decompress_kernel");
        rc != H2_OK)
      return rc;
    if (int rc = launched(ops->ipa_replay(k_, M, base + o_states, base + o_points, base + o_pstatus, base + o_scalars, base + o_replay,
                                          base + o_status, nullptr, stream),
                          "ipa_replay_kernel");
        rc != H2_OK)
      return rc;
    std::vector<uint8_t> status(M);
    H2_TRY(hipMemcpyAsync(status.data(), base + o_status, M, hipMemcpyDeviceToHost, stream));
    H2_TRY(hipStreamSynchronize(stream));
    std::vector<size_t> live;                              // device proofs whose replay went through
    for (size_t j = 0; j < M; j++)
      if (status[j] == 0) live.push_back(j);

    int rc = H2_OK;
    size_t checks = 0;
    std::vector<uint32_t> weights(M * IPA_WEIGHT_WORDS);
    // sum_p w_p (sum [1/u_j] L_j + P + [xi] S + sum [u_j] R_j - [v] G[0] - [c] <s, G> - [c b0 z] U - [f] W) == 0 over the subset
    auto check = [&](const size_t* subset, size_t cnt) -> bool {
      if (rc != H2_OK) return false;
      checks++;
      std::fill(weights.begin(), weights.end(), 0u);
      for (size_t s = 0; s < cnt; s++) {
        uint32_t* w = &weights[subset[s] * IPA_WEIGHT_WORDS];
        uint8_t raw[16];
        do {
          if (rng) {
            rng(rng_ctx, raw, 16);
          } else {
            for (size_t got = 0; got < 16;) {
              const ssize_t r = getrandom(raw + got, 16 - got, 0);
              if (r <= 0) {
                g_h2.last_error = "getrandom failed";
                rc = H2_EDEVICE;
                return false;
              }
              got += (size_t)r;
            }
          }
          for (int i = 0; i < 4; i++)
            w[i] = (uint32_t)raw[4 * i] | ((uint32_t)raw[4 * i + 1] << 8) | ((uint32_t)raw[4 * i + 2] << 16) | ((uint32_t)raw[4 * i + 3] << 24);
        } while (!(w[0] | w[1] | w[2] | w[3]));
        w[4] = (uint32_t)s;
      }
      auto step = [&](int st) {
        if (rc == H2_OK) rc = st;
        return rc == H2_OK;
      };
      auto copied = [&](hipError_t e, const char* what) { return e == hipSuccess ? (int)H2_OK : dev_fail(e, what); };
      char* jac = base + o_jac;
      if (!step(copied(hipMemcpyAsync(base + o_weights, weights.data(), weights.size() * 4, hipMemcpyHostToDevice, stream), "weights")))
        return false;
      if (!step(launched(ops->ipa_verify_prepare(base + o_replay, base + o_x3, base + o_v, base + o_weights, base + o_scal, base + o_table,
                                                 base + o_terms, k_, M, stream),
                         "ipa_verify_prepare_kernel")))
        return false;
      if (!step(ipa_sum_run(ops, base + o_table, cnt, k_, base + o_col, false, stream))) return false;
      if (!step(launched(ops->ipa_verify_finish(base + o_terms, M, base + o_col, k_, stream), "ipa_verify_finish_kernel"))) return false;
      if (!step(msm_device_run(*k.c, (int)curve, *be, base + o_col, 0, n + 2, n + 2, 1, jac, false, stream))) return false;
      if (!step(msm_points_run(*k.c, (int)curve, base + o_points, base + o_scal, G + M, G + M, 1, jac + 96, stream))) return false;
      if (!step(launched(ops->points_sum(jac, jac + 192, 2, 1, stream), "points_sum_kernel"))) return false;
      uint64_t total[12];
      if (!step(copied(hipMemcpyAsync(total, jac + 192, 96, hipMemcpyDeviceToHost, stream), "the check's sum"))) return false;
      if (!step(copied(hipStreamSynchronize(stream), "hipStreamSynchronize"))) return false;
      return !(total[8] | total[9] | total[10] | total[11]);
    };
    // the verdicts of a subset; known_bad: a combined check has already shown that it holds a culprit
    std::function<void(const size_t*, size_t, bool)> settle = [&](const size_t* subset, size_t cnt, bool known_bad) {
      if (rc != H2_OK) return;
      if (!known_bad && check(subset, cnt)) {
        for (size_t s = 0; s < cnt; s++) ok[item[subset[s]]] = 1;
        return;
      }
      if (cnt == 1) return;                                // a singleton's verdict is its own equation; w != 0
      const size_t half = cnt / 2;
      if (check(subset, half)) {
        for (size_t s = 0; s < half; s++) ok[item[subset[s]]] = 1;
        settle(subset + half, cnt - half, cnt - half > 1); // the culprits are on the other side; one alone is still checked
      } else {
        settle(subset, half, true);
        settle(subset + half, cnt - half, false);
      }
    };
    if (!live.empty()) settle(live.data(), live.size(), false);
    if (rc != H2_OK) return rc;
    if (checks_out) *checks_out = checks;
    if (all_ok) {
      *all_ok = 1;
      for (size_t i = 0; i < count; i++)
        if (!ok[i]) *all_ok = 0;
    }
    return A.wait();
  } catch (const std::bad_alloc&) {
    g_h2.last_error = "ipa: no host memory for the batch";
    return H2_ENOMEM;
  }
}

// ---- the IPA prover behind one call (h2_ipa_prove.hpp) --------------------------------------------------------------------
int h2_ipa_prove_state_bytes(uint32_t k, size_t m, size_t* out) {
  if (k == 0 || k > IPA_MAX_K || m == 0 || m > IPA_MAX_BATCH || !out) return H2_EINVAL;
  *out = IpaProveLayout(k, m).total;
  return H2_OK;
}

}  // extern "C"

namespace {
// h2_ipa_prove_rounds_device behind its Call: every refusal first, then ONE upload -- the scalar table as begin and round 0
// read it, every blind, f, the midstates: one range of the state -- and begin, k x (round, MSM, step), final, step.  No
// synchronisation and nothing read back
int ipa_prove_rounds_run(DevCtx& c, hipStream_t stream, int curve, uint64_t bases, uint32_t k_, size_t m, const void* const* d_p,
                         const uint64_t* x3, const uint64_t* z, const uint64_t* f0, const uint64_t* round_blinds,
                         const h2_transcript_state_t* states, void* d_state, void* d_tail, void* d_states_out, void* d_status) {
  if (!curve_ok(curve) || !ops_of(curve)->ipa_prove_step || k_ == 0 || k_ > IPA_MAX_K || m == 0 || m > IPA_MAX_BATCH) return H2_EINVAL;
  if (!d_p || !x3 || !z || !f0 || !round_blinds || !states) return H2_EINVAL;
  if (!ipa_dev_ptr(d_state) || !ipa_dev_ptr(d_tail) || !d_status || ((uintptr_t)d_status & 3) || (d_states_out && ((uintptr_t)d_states_out & 15)))
    return H2_EINVAL;
  for (size_t i = 0; i < m; i++)
    if (!ipa_dev_ptr(d_p[i]) || states[i].buflen > 128) return H2_EINVAL;
  if (!H2_BY_SCALAR_FIELD(curve, ipa_canonical)(x3, m) || !H2_BY_SCALAR_FIELD(curve, ipa_canonical)(z, m) ||
      !H2_BY_SCALAR_FIELD(curve, ipa_canonical)(f0, m) || !H2_BY_SCALAR_FIELD(curve, ipa_canonical)(round_blinds, 2 * k_ * m))
    return H2_EINVAL;
  const IpaBatchLayout L(k_, m);
  const IpaProveLayout P(k_, m);
  const BasesEntry* be = nullptr;
  if (int rc = msm_common_checks(curve, bases, 0, L.col_stride, 2 * m, &be); rc != H2_OK) return rc;
  if (be->n != L.col_stride) return H2_EINVAL;          // exactly G || U || W
  if (int rc = msm_device_plan_check(*be, L.col_stride, L.col_stride, 2 * m); rc != H2_OK) return rc;

  const size_t up0 = L.scal * 32, row = m * 32;
  std::vector<uint8_t> host;
  try {
    host.assign(P.lr - up0, 0);
  } catch (const std::bad_alloc&) {
    g_h2.last_error = "ipa: no host memory for the call's scalars";
    return H2_ENOMEM;
  }
  memcpy(&host[0], x3, row);                             // row 0: begin's x3; row 1: the m pointers d_p
  for (size_t i = 0; i < m; i++) {
    const uint64_t p = (uint64_t)(uintptr_t)d_p[i];
    memcpy(&host[row + 8 * i], &p, 8);
    memcpy(&host[3 * row + 32 * i], round_blinds + 4 * (i * 2 * k_), 32);       // rows 3, 4: l_0, r_0
    memcpy(&host[4 * row + 32 * i], round_blinds + 4 * (i * 2 * k_ + 1), 32);
  }
  memcpy(&host[2 * row], z, row);                        // row 2 stands for the whole call
  memcpy(&host[P.blinds - up0], round_blinds, 2 * k_ * row);
  memcpy(&host[P.f - up0], f0, row);
  memcpy(&host[P.states - up0], states, m * sizeof(h2_transcript_state_t));
  char* st = (char*)d_state;
  // a pageable source: the runtime has read `host` when the call returns (it stages the bytes or waits for the copy)
  H2_TRY(hipMemcpyAsync(st + up0, host.data(), host.size(), hipMemcpyHostToDevice, stream));

  const CurveOps* ops = ops_of(curve);
  IpaOne one;
  memset(&one, 0, sizeof one);
  one.table = 1;                                         // the step kernel makes the scalars: the table at m = 1 too
  const int inv = g_knobs.ipa_inv_form;
  if (int rc = launched(ops->ipa_begin(k_, m, one, d_state, stream), "ipa_begin_kernel"); rc != H2_OK) return rc;
  for (uint32_t j = 0; j < k_; j++) {
    if (int rc = launched(ops->ipa_round(k_, j, m, one, d_state, stream), "ipa_round_kernel"); rc != H2_OK) return rc;
    if (int rc = msm_device_run(c, curve, *be, st + L.col * 32, 0, L.col_stride, L.col_stride, 2 * m, st + P.lr, true, stream); rc != H2_OK)
      return rc;
    if (int rc = launched(ops->ipa_prove_step(k_, j, m, d_state, d_tail, nullptr, d_status, inv, stream), "ipa_prove_step_kernel"); rc != H2_OK)
      return rc;
  }
  if (int rc = launched(ops->ipa_final(k_, m, one, d_state, st + P.lr, nullptr, stream), "ipa_final_kernel"); rc != H2_OK) return rc;
  return launched(ops->ipa_prove_step(k_, k_, m, d_state, d_tail, d_states_out, d_status, inv, stream), "ipa_prove_step_kernel");
}

// S (affine, Montgomery limbs, (0, 0) the identity) onto a transcript: its wire form, then xi and z squeezed (Montgomery
// limbs); the state is left behind the two challenges
template <class CV>
void ipa_absorb_commitment(const uint64_t aff[8], h2_transcript_state_t* state, uint8_t wire[32], uint64_t xi[4], uint64_t z[4]) {
  uint8_t msg[65];
  msg[0] = 1;
  HF<typename CV::Base>::from_mont_limbs(aff).to_le_bytes(msg + 1);
  HF<typename CV::Base>::from_mont_limbs(aff + 4).to_le_bytes(msg + 33);
  memcpy(wire, msg + 1, 32);
  wire[31] |= (uint8_t)((msg[33] & 1) << 7);
  Blake2b b;
  b.import_state((const uint8_t*)state);
  b.update(msg, 65);
  for (uint64_t* out : {xi, z}) {
    const uint8_t zero = 0;
    uint8_t digest[64];
    b.update(&zero, 1);
    b.digest(digest);
    transcript_reduce<typename CV::Scalar>(digest, out);
  }
  b.export_state((uint8_t*)state);
}

template <class FP>
void ipa_one_limbs(uint64_t out[4]) {
  HF<FP>::one().mont_limbs(out);
}

// s_blind xi + p_blind on Montgomery limbs
template <class FP>
void ipa_f0(const uint64_t s_blind[4], const uint64_t xi[4], const uint64_t p_blind[4], uint64_t out[4]) {
  (HF<FP>::from_mont_limbs(s_blind) * HF<FP>::from_mont_limbs(xi) + HF<FP>::from_mont_limbs(p_blind)).mont_limbs(out);
}
}  // namespace

extern "C" {

int h2_ipa_prove_rounds_device(h2_curve_t curve, uint64_t bases, uint32_t k_, size_t m, const void* const* d_p, const uint64_t* x3,
                               const uint64_t* z, const uint64_t* f0, const uint64_t* round_blinds,
                               const h2_transcript_state_t* states, void* d_state, void* d_tail, void* d_states_out, void* d_status,
                               void* stream_) {
  Call k(stream_);
  if (k.rc != H2_OK) return k.rc;
  return ipa_prove_rounds_run(*k.c, k.stream, (int)curve, bases, k_, m, d_p, x3, z, f0, round_blinds, states, d_state, d_tail,
                              d_states_out, d_status);
}

int h2_ipa_create_proofs(h2_curve_t curve, uint64_t bases, uint32_t k_, size_t m, const h2_transcript_state_t* states,
                         const void* const* d_p, const uint64_t* p_blind, const uint64_t* x3, const void* const* d_s_poly,
                         const uint8_t* seeds, const uint64_t* s_blind, const uint64_t* round_blinds, uint8_t* proofs,
                         h2_transcript_state_t* states_out, uint32_t* status) {
  Call k(nullptr);
  if (k.rc != H2_OK) return k.rc;
  const int cv = (int)curve;
  if (!curve_ok(cv) || !ops_of(cv)->ipa_prove_step || k_ == 0 || k_ > IPA_MAX_K || m == 0 || m > IPA_MAX_BATCH) return H2_EINVAL;
  if (!states || !d_p || !p_blind || !x3 || !d_s_poly || !s_blind || !round_blinds || !proofs || !status) return H2_EINVAL;
  for (size_t i = 0; i < m; i++) {
    if (!ipa_dev_ptr(d_p[i]) || states[i].buflen > 128) return H2_EINVAL;
    if (d_s_poly[i] ? ((uintptr_t)d_s_poly[i] & 15) != 0 : !seeds) return H2_EINVAL;
  }
  if (!H2_BY_SCALAR_FIELD(cv, ipa_canonical)(p_blind, m) || !H2_BY_SCALAR_FIELD(cv, ipa_canonical)(x3, m) ||
      !H2_BY_SCALAR_FIELD(cv, ipa_canonical)(s_blind, m) || !H2_BY_SCALAR_FIELD(cv, ipa_canonical)(round_blinds, 2 * k_ * m))
    return H2_EINVAL;
  const size_t n = (size_t)1 << k_, rows = n + 2, per = 2 * (size_t)k_ + 2;
  const BasesEntry* be = nullptr;
  if (int rc = msm_common_checks(cv, bases, 0, rows, 2 * m, &be); rc != H2_OK) return rc;
  if (be->n != rows) return H2_EINVAL;                   // exactly G || U || W
  if (int rc = msm_device_plan_check(*be, rows, rows, m); rc != H2_OK) return rc;
  if (int rc = msm_device_plan_check(*be, rows, rows, 2 * m); rc != H2_OK) return rc;

  DevCtx& c = *k.c;
  hipStream_t stream = k.stream;
  // the scratch: the columns s_poly_i || 0 || s_blind_i, the polynomials p'_i, the prove state, and what is read back at the
  // end as one range: the tails, the midstates, the status words
  size_t off = 0;
  auto region = [&](size_t bytes) { const size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; };
  const size_t o_cols = region(m * rows * 32), o_pp = region(m * n * 32), o_vals = region(2 * m * 32), o_aff = region(m * 64),
               o_state = region(IpaProveLayout(k_, m).total), o_tail = off, back_tail = m * per * 32,
               back_states = m * sizeof(h2_transcript_state_t), back = back_tail + back_states + m * 4;
  region(back);
  ArenaLease A(c.stage, off, stream);
  if (A.rc != H2_OK) return A.rc;
  char* base = (char*)A.a.p;
  try {
    // 1. the columns: s_poly_i given or expanded from its seed; the blind in row n + 1, zero in row n
    std::vector<uint64_t> tails(8 * m, 0);
    for (size_t i = 0; i < m; i++) memcpy(&tails[8 * i + 4], s_blind + 4 * i, 32);
    H2_TRY(hipMemcpy2DAsync(base + o_cols + n * 32, rows * 32, tails.data(), 64, 64, m, hipMemcpyHostToDevice, stream));
    std::vector<const void*> ptrs(2 * m);
    for (size_t i = 0; i < m; i++) {
      char* col = base + o_cols + i * rows * 32;
      if (d_s_poly[i]) {
        H2_TRY(hipMemcpyAsync(col, d_s_poly[i], n * 32, hipMemcpyDeviceToDevice, stream));
      } else {
        if (int rc = h2_chacha20_scalars_device(curve, seeds + 32 * i, 0, n, col, stream); rc != H2_OK) return rc;
      }
      ptrs[i] = col;
      ptrs[m + i] = d_p[i];
    }
    // 2. s_poly_i(x3_i) and p_i(x3_i): the first of the call's three synchronisations
    std::vector<uint64_t> points(8 * m), vals(8 * m);
    memcpy(&points[0], x3, m * 32);
    memcpy(&points[4 * m], x3, m * 32);
    if (int rc = poly_eval_enqueue(c, cv, ptrs.data(), n, points.data(), 2 * m, base + o_vals, stream); rc != H2_OK) return rc;
    H2_TRY(hipMemcpyAsync(vals.data(), base + o_vals, 2 * m * 32, hipMemcpyDeviceToHost, stream));
    H2_TRY(hipStreamSynchronize(stream));
    // 3. s_poly_i[0] -= s_poly_i(x3_i), then the m commitments S_i: the second synchronisation
    std::vector<h2_lincomb_job_t> jobs(m);
    std::vector<h2_lincomb_term_t> terms(2 * m);
    uint64_t one_limbs[4];
    H2_BY_SCALAR_FIELD(cv, ipa_one_limbs)(one_limbs);
    for (size_t i = 0; i < m; i++) {
      jobs[i] = h2_lincomb_job_t{base + o_cols + i * rows * 32, (uint32_t)i, 1, (uint32_t)i, 1, 0, 0};
      terms[i].d_poly = jobs[i].d_out;
      memcpy(terms[i].coeff, one_limbs, 32);
    }
    if (int rc = h2_poly_lincomb_device(curve, jobs.data(), m, terms.data(), m, vals.data(), m, nullptr, 0, n, stream); rc != H2_OK) return rc;
    if (int rc = msm_device_run(c, cv, *be, base + o_cols, 0, rows, rows, m, base + o_aff, true, stream); rc != H2_OK) return rc;
    std::vector<uint64_t> aff(8 * m);
    H2_TRY(hipMemcpyAsync(aff.data(), base + o_aff, m * 64, hipMemcpyDeviceToHost, stream));
    H2_TRY(hipStreamSynchronize(stream));
    // 4. S onto the transcripts, xi and z off them; p'_i = xi_i s_poly_i + p_i, p'_i[0] -= p_i(x3_i); f_i = s_blind_i xi_i + p_blind_i
    std::vector<h2_transcript_state_t> mid(states, states + m);
    std::vector<uint64_t> xi(4 * m), z(4 * m), f0(4 * m);
    std::vector<const void*> d_pp(m);
    for (size_t i = 0; i < m; i++) {
      uint8_t* wire = proofs + i * (per + 1) * 32;
      if (cv == H2_PALLAS)
        ipa_absorb_commitment<PALLAS_CURVE>(&aff[8 * i], &mid[i], wire, &xi[4 * i], &z[4 * i]);
      else
        ipa_absorb_commitment<VESTA_CURVE>(&aff[8 * i], &mid[i], wire, &xi[4 * i], &z[4 * i]);
      H2_BY_SCALAR_FIELD(cv, ipa_f0)(s_blind + 4 * i, &xi[4 * i], p_blind + 4 * i, &f0[4 * i]);
      d_pp[i] = base + o_pp + i * n * 32;
      jobs[i] = h2_lincomb_job_t{base + o_pp + i * n * 32, (uint32_t)(2 * i), 2, (uint32_t)i, 1, 0, 0};
      terms[2 * i].d_poly = base + o_cols + i * rows * 32;
      memcpy(terms[2 * i].coeff, &xi[4 * i], 32);
      terms[2 * i + 1].d_poly = d_p[i];
      memcpy(terms[2 * i + 1].coeff, one_limbs, 32);
    }
    if (int rc = h2_poly_lincomb_device(curve, jobs.data(), m, terms.data(), 2 * m, &vals[4 * m], m, nullptr, 0, n, stream); rc != H2_OK)
      return rc;
    // 5. the rounds, nothing through the host; one read-back behind them: the third synchronisation
    if (int rc = ipa_prove_rounds_run(c, stream, cv, bases, k_, m, d_pp.data(), x3, z.data(), f0.data(), round_blinds, mid.data(),
                                      base + o_state, base + o_tail, base + o_tail + back_tail, base + o_tail + back_tail + back_states);
        rc != H2_OK)
      return rc;
    std::vector<uint8_t> out(back);
    H2_TRY(hipMemcpyAsync(out.data(), base + o_tail, back, hipMemcpyDeviceToHost, stream));
    if (int rc = A.wait(); rc != H2_OK) return rc;
    for (size_t i = 0; i < m; i++) memcpy(proofs + (i * (per + 1) + 1) * 32, &out[i * per * 32], per * 32);
    if (states_out) memcpy(states_out, &out[back_tail], back_states);
    memcpy(status, &out[back_tail + back_states], m * 4);
    return H2_OK;
  } catch (const std::bad_alloc&) {
    g_h2.last_error = "ipa: no host memory for the batch";
    return H2_ENOMEM;
  }
}

// ---- Poseidon over resident columns (h2_poseidon.hpp, h2_poseidon_merkle.hpp) -----------------------------------------------
// One body per operation, the width an argument: the h2_poseidon_X names are the h2_poseidon_wide_X calls at width 3.
static_assert(H2_POSEIDON_MAX_ROUNDS == POSEIDON_MAX_ROUNDS, "the header states the kernels' maximum");
static_assert(H2_MERKLE_OK == MERKLE_OK && H2_MERKLE_RANGE == MERKLE_RANGE && H2_MERKLE_NONCANONICAL == MERKLE_NONCANONICAL &&
                  H2_MERKLE_SUPERSEDED == MERKLE_SUPERSEDED && H2_MERKLE_MISMATCH == MERKLE_MISMATCH,
              "the header states the kernels' status words");
namespace {
// hashes below which a width-3 launch runs one permutation on four lanes, unless a test knob fixes the form
size_t poseidon_walk_quad_max() { return g_knobs.poseidon_walk_form == 1 ? 0 : g_knobs.poseidon_walk_form == 2 ? SIZE_MAX : POSEIDON_WALK_QUAD_MAX; }
// depth >= 1 and a^depth <= 2^30
bool poseidon_depth_ok(uint32_t width, uint32_t depth) { return depth >= 1 && depth <= 30 / merkle_lg(width); }
struct Span {
  const void* p;
  size_t bytes;
};
// does a written range overlap a range that is read, or another one that is written?  (absent and empty ranges aside)
bool merkle_overlap(std::initializer_list<Span> outs, std::initializer_list<Span> ins) {
  auto hit = [](const Span& a, const Span& b) { return a.p && b.p && a.bytes && b.bytes && poseidon_overlap(a.p, a.bytes, b.p, b.bytes); };
  for (auto o = outs.begin(); o != outs.end(); ++o) {
    for (const Span& x : ins)
      if (hit(*o, x)) return true;
    for (auto o2 = o + 1; o2 != outs.end(); ++o2)
      if (hit(*o, *o2)) return true;
  }
  return false;
}
}  // namespace

int h2_poseidon_merkle_tail(void) { return (int)(g_knobs.poseidon_merkle_tail ? g_knobs.poseidon_merkle_tail : POSEIDON_MERKLE_TAIL); }

int h2_poseidon_wide_constants(h2_curve_t curve, uint32_t width, uint32_t r_f, uint32_t r_p, uint64_t* out, size_t cap_elems,
                               size_t* n_elems) {
  if (!curve_ok((int)curve) || !poseidon_width_ok(width) || !poseidon_rounds_ok(r_f, r_p) || !n_elems) return H2_EINVAL;
  const size_t need = poseidon_dense_elems(width, r_f, r_p);
  *n_elems = need;
  if (!out || cap_elems < need) return H2_EINVAL;
  (void)poseidon_wide_table_mont((int)curve, width, r_f, r_p, false, out);
  return H2_OK;
}
int h2_poseidon_constants(h2_curve_t curve, uint32_t r_f, uint32_t r_p, uint64_t* out, size_t cap_elems, size_t* n_elems) {
  return h2_poseidon_wide_constants(curve, 3, r_f, r_p, out, cap_elems, n_elems);
}

int h2_poseidon_wide_permute_device(h2_curve_t curve, uint32_t width, uint32_t r_f, uint32_t r_p, const void* d_in, void* d_out, size_t n,
                                    void* stream_) {
  Call k(stream_);
  if (k.rc != H2_OK) return k.rc;
  if (!curve_ok((int)curve) || !poseidon_width_ok(width) || !poseidon_rounds_ok(r_f, r_p) || !poseidon_dev_ptr(d_in) ||
      !poseidon_dev_ptr(d_out) || n > ((size_t)1 << 40))
    return H2_EINVAL;
  if (d_out != d_in && poseidon_overlap(d_in, 32 * width * n, d_out, 32 * width * n)) return H2_EINVAL;
  if (n == 0) return H2_OK;
  const void* table = nullptr;
  if (int rc = poseidon_table_get(*k.c, (int)curve, width, r_f, r_p, &table); rc != H2_OK) return rc;
  // the partial rounds: the width's own form, unless a test knob fixes it (1: dense, 2: sparse)
  return launched(poseidon_ops_of((int)curve)->permute(width, g_knobs.poseidon_wide_form, d_in, d_out, n, table, r_f, r_p, k.stream),
                  "poseidon_permute_kernel");
}
int h2_poseidon_permute_device(h2_curve_t curve, uint32_t r_f, uint32_t r_p, const void* d_in, void* d_out, size_t n, void* stream_) {
  return h2_poseidon_wide_permute_device(curve, 3, r_f, r_p, d_in, d_out, n, stream_);
}

int h2_poseidon_wide_hash_device(h2_curve_t curve, uint32_t width, uint32_t r_f, uint32_t r_p, const void* d_msgs, size_t len,
                                 size_t msg_stride, size_t n, void* d_out, void* stream_) {
  Call k(stream_);
  if (k.rc != H2_OK) return k.rc;
  if (!curve_ok((int)curve) || !poseidon_width_ok(width) || !poseidon_rounds_ok(r_f, r_p) || !poseidon_dev_ptr(d_msgs) ||
      !poseidon_dev_ptr(d_out) || len == 0 || len > 65535 || msg_stride < len || msg_stride > ((size_t)1 << 32) || n > ((size_t)1 << 40))
    return H2_EINVAL;
  if (n == 0) return H2_OK;
  if (poseidon_overlap(d_msgs, 32 * ((n - 1) * msg_stride + len), d_out, 32 * n)) return H2_EINVAL;
  const void* table = nullptr;
  if (int rc = poseidon_table_get(*k.c, (int)curve, width, r_f, r_p, &table); rc != H2_OK) return rc;
  uint64_t cap[4];
  H2_BY_SCALAR_FIELD((int)curve, poseidon_capacity_t)(len, cap);
  return launched(poseidon_ops_of((int)curve)->hash(width, d_msgs, (uint32_t)len, msg_stride, n, d_out, cap, table, r_f, r_p,
                                                    poseidon_chain_min_n(), k.stream),
                  "poseidon_hash_kernel");
}
int h2_poseidon_hash_device(h2_curve_t curve, uint32_t r_f, uint32_t r_p, const void* d_msgs, size_t len, size_t msg_stride, size_t n,
                            void* d_out, void* stream_) {
  return h2_poseidon_wide_hash_device(curve, 3, r_f, r_p, d_msgs, len, msg_stride, n, d_out, stream_);
}

int h2_poseidon_wide_merkle_device(h2_curve_t curve, uint32_t width, uint32_t r_f, uint32_t r_p, const void* d_leaves, uint32_t depth,
                                   void* d_nodes, void* stream_) {
  Call k(stream_);
  if (k.rc != H2_OK) return k.rc;
  if (!curve_ok((int)curve) || !poseidon_width_ok(width) || !poseidon_rounds_ok(r_f, r_p) || !poseidon_dev_ptr(d_leaves) ||
      !poseidon_dev_ptr(d_nodes) || !poseidon_depth_ok(width, depth))
    return H2_EINVAL;
  const uint32_t lg = merkle_lg(width);
  const size_t leaves = merkle_pow(lg, depth), nodes = merkle_level_offset(lg, depth, depth);
  if (poseidon_overlap(d_leaves, 32 * leaves, d_nodes, 32 * nodes)) return H2_EINVAL;
  const void* table = nullptr;
  if (int rc = poseidon_table_get(*k.c, (int)curve, width, r_f, r_p, &table); rc != H2_OK) return rc;
  uint64_t cap[4];
  H2_BY_SCALAR_FIELD((int)curve, poseidon_capacity_t)(width - 1, cap);
  return launched(poseidon_ops_of((int)curve)->merkle(width, d_leaves, depth, d_nodes, cap, table, r_f, r_p,
                                                      (uint32_t)h2_poseidon_merkle_tail(), poseidon_chain_min_n(), k.stream),
                  "poseidon_merkle kernels");
}
int h2_poseidon_merkle_device(h2_curve_t curve, uint32_t r_f, uint32_t r_p, const void* d_leaves, uint32_t depth, void* d_nodes,
                              void* stream_) {
  return h2_poseidon_wide_merkle_device(curve, 3, r_f, r_p, d_leaves, depth, d_nodes, stream_);
}

int h2_poseidon_wide_merkle_paths_device(h2_curve_t curve, uint32_t width, const void* d_leaves, const void* d_nodes, uint32_t depth,
                                         const void* d_indices, size_t n, void* d_paths, void* d_status, void* stream_) {
  Call k(stream_);
  if (k.rc != H2_OK) return k.rc;
  if (!curve_ok((int)curve) || !poseidon_width_ok(width) || !poseidon_depth_ok(width, depth) || n > ((size_t)1 << 31) ||
      !poseidon_dev_ptr(d_leaves) || !poseidon_dev_ptr(d_nodes) || !poseidon_dev_ptr(d_indices) || !poseidon_dev_ptr(d_paths) ||
      !poseidon_dev_ptr(d_status))
    return H2_EINVAL;
  const uint32_t lg = merkle_lg(width);
  const size_t leaves = merkle_pow(lg, depth), nodes = merkle_level_offset(lg, depth, depth);
  const Span paths{d_paths, 32 * n * depth * (width - 2)}, status{d_status, 4 * n};
  if (merkle_overlap({paths, status}, {Span{d_leaves, 32 * leaves}, Span{d_nodes, 32 * nodes}, Span{d_indices, 4 * n}})) return H2_EINVAL;
  if (n == 0) return H2_OK;
  return launched(poseidon_ops_of((int)curve)->paths(width, d_leaves, d_nodes, depth, d_indices, n, d_paths, d_status, k.stream),
                  "poseidon_merkle_paths_kernel");
}
int h2_poseidon_merkle_paths_device(h2_curve_t curve, const void* d_leaves, const void* d_nodes, uint32_t depth, const void* d_indices,
                                    size_t n, void* d_paths, void* d_status, void* stream_) {
  return h2_poseidon_wide_merkle_paths_device(curve, 3, d_leaves, d_nodes, depth, d_indices, n, d_paths, d_status, stream_);
}

int h2_poseidon_wide_merkle_verify_device(h2_curve_t curve, uint32_t width, uint32_t r_f, uint32_t r_p, const void* d_leaf_values,
                                          const void* d_indices, const void* d_paths, uint32_t depth, size_t n, const void* d_root,
                                          void* d_roots_out, void* d_status, void* stream_) {
  Call k(stream_);
  if (k.rc != H2_OK) return k.rc;
  if (!curve_ok((int)curve) || !poseidon_width_ok(width) || !poseidon_depth_ok(width, depth) || n > ((size_t)1 << 31) ||
      !poseidon_rounds_ok(r_f, r_p) || !poseidon_dev_ptr(d_leaf_values) || !poseidon_dev_ptr(d_indices) || !poseidon_dev_ptr(d_paths) ||
      !poseidon_dev_ptr(d_status) || ((uintptr_t)d_root & 15) || ((uintptr_t)d_roots_out & 15))
    return H2_EINVAL;
  const Span roots{d_roots_out, 32 * n}, status{d_status, 4 * n};
  if (merkle_overlap({roots, status}, {Span{d_leaf_values, 32 * n}, Span{d_indices, 4 * n},
                                       Span{d_paths, 32 * n * depth * (width - 2)}, Span{d_root, 32}}))
    return H2_EINVAL;
  if (n == 0) return H2_OK;
  const void* table = nullptr;
  if (int rc = poseidon_table_get(*k.c, (int)curve, width, r_f, r_p, &table); rc != H2_OK) return rc;
  uint64_t cap[4];
  H2_BY_SCALAR_FIELD((int)curve, poseidon_capacity_t)(width - 1, cap);
  return launched(poseidon_ops_of((int)curve)->verify(width, d_leaf_values, d_indices, d_paths, depth, n, d_root, d_roots_out, d_status,
                                                      cap, table, r_f, r_p, poseidon_walk_quad_max(), k.stream),
                  "poseidon_merkle_verify_kernel");
}
int h2_poseidon_merkle_verify_device(h2_curve_t curve, uint32_t r_f, uint32_t r_p, const void* d_leaf_values, const void* d_indices,
                                     const void* d_paths, uint32_t depth, size_t n, const void* d_root, void* d_roots_out, void* d_status,
                                     void* stream_) {
  return h2_poseidon_wide_merkle_verify_device(curve, 3, r_f, r_p, d_leaf_values, d_indices, d_paths, depth, n, d_root, d_roots_out,
                                               d_status, stream_);
}

// binary trees only
int h2_poseidon_merkle_update_device(h2_curve_t curve, uint32_t r_f, uint32_t r_p, void* d_leaves, void* d_nodes, uint32_t depth,
                                     const void* d_indices, const void* d_values, size_t n, void* d_status, void* stream_) {
  Call k(stream_);
  if (k.rc != H2_OK) return k.rc;
  if (!curve_ok((int)curve) || !poseidon_depth_ok(3, depth) || n > ((size_t)1 << 31) || !poseidon_rounds_ok(r_f, r_p) ||
      !poseidon_dev_ptr(d_leaves) || !poseidon_dev_ptr(d_nodes) || !poseidon_dev_ptr(d_indices) || !poseidon_dev_ptr(d_values) ||
      !poseidon_dev_ptr(d_status))
    return H2_EINVAL;
  const size_t leaves = (size_t)1 << depth;
  const Span lv{d_leaves, 32 * leaves}, nd{d_nodes, 32 * (leaves - 1)}, status{d_status, 4 * n};
  if (merkle_overlap({lv, nd, status}, {Span{d_indices, 4 * n}, Span{d_values, 32 * n}})) return H2_EINVAL;
  if (n == 0) return H2_OK;
  const PoseidonOps* ops = poseidon_ops_of((int)curve);
  const size_t scratch = ops->update_scratch(n, depth);
  if (scratch == 0) {
    g_h2.last_error = "poseidon merkle update: the sort gave no scratch size";
    return H2_EDEVICE;
  }
  const void* table = nullptr;
  if (int rc = poseidon_table_get(*k.c, (int)curve, 3, r_f, r_p, &table); rc != H2_OK) return rc;
  uint64_t cap2[4];
  H2_BY_SCALAR_FIELD((int)curve, poseidon_capacity_t)(2, cap2);
  ArenaLease A(k.c->div_ws, scratch, k.stream);
  if (A.rc != H2_OK) return A.rc;
  if (int rc = launched(ops->update(d_leaves, d_nodes, depth, d_indices, d_values, n, d_status, cap2, table, r_f, r_p,
                                    poseidon_walk_quad_max(), A.a.p, A.a.bytes, k.stream),
                        "poseidon_merkle_update kernels");
      rc != H2_OK)
    return rc;
  return A.release();
}

int h2_poly_pointwise_device(h2_curve_t curve, int op, void* d_a, const void* d_b, size_t n, void* stream_) {
  Call k(stream_);
  if (k.rc != H2_OK) return k.rc;
  if (!curve_ok((int)curve) || !d_a || !d_b || op < 0 || op > 2) return H2_EINVAL;
  if (n == 0) return H2_OK;
  return launched(ops_of((int)curve)->poly_pointwise(d_a, d_b, n, op, k.stream), "poly_pointwise_kernel");
}

// host columns; with several contexts column j is transformed by context j mod G (a single NTT is not split:
// "replicas only")
int h2_ntt_batch(h2_curve_t curve, uint64_t* const* cols, size_t m, const uint64_t omega[4], uint32_t log_n) {
  std::lock_guard<std::recursive_mutex> lk(g_h2_mu);
  if (!g_h2.ready) return H2_ENOTINIT;
  if (!curve_ok((int)curve) || !cols || !omega || m == 0 || log_n > 30) return H2_EINVAL;
  for (size_t j = 0; j < m; j++)
    if (!cols[j]) return H2_EINVAL;
  if (log_n == 0) return H2_OK;
  const size_t col_bytes = (size_t)32 << log_n;
  const size_t G = g_h2.ctx.size();
  std::vector<std::optional<ArenaLease>> stages(G);
  for (size_t g = 0; g < G && g < m; g++) {
    DevCtx& c = g_h2.ctx[g];
    DeviceGuard dg(c.device);
    const size_t mine = (m - g + G - 1) / G;
    if (int st = stages[g].emplace(c.stage, mine * col_bytes, c.stream).rc; st != H2_OK) return st;
    for (size_t i = 0; i < mine; i++)
      H2_TRY(hipMemcpyAsync((char*)c.stage.p + i * col_bytes, cols[g + i * G], col_bytes, hipMemcpyHostToDevice,
                            c.stream));
    int rc = ntt_enqueue(c, (int)curve, c.stage.p, mine, omega, log_n, c.stream);
    if (rc != H2_OK) return rc;
    for (size_t i = 0; i < mine; i++)
      H2_TRY(hipMemcpyAsync(cols[g + i * G], (char*)c.stage.p + i * col_bytes, col_bytes, hipMemcpyDeviceToHost,
                            c.stream));
  }
  for (size_t g = 0; g < G && g < m; g++) {
    DeviceGuard dg(g_h2.ctx[g].device);
    if (int st = stages[g]->wait(); st != H2_OK) return st;
  }
  return H2_OK;
}

// best_fft over group elements (FftGroup for C::Curve): n = 2^log_n Jacobian points in place, natural order, unscaled
int h2_fft_group_device(h2_curve_t curve, void* d_points_jac, const uint64_t omega[4], uint32_t log_n, void* stream_) {
  Call k(stream_);
  if (k.rc != H2_OK) return k.rc;
  if (!curve_ok((int)curve) || !d_points_jac || !omega || log_n > 26) return H2_EINVAL;
  if (log_n == 0) return H2_OK;
  const CurveOps* ops = ops_of((int)curve);
  ArenaLease A(k.c->msm_ws.of(k.stream), ops->group_fft_scratch(log_n), k.stream);      // the MSM workspace, idle here
  if (A.rc != H2_OK) return A.rc;
  if (int rc = launched(ops->group_fft(d_points_jac, d_points_jac, A.a.p, omega, log_n, g_knobs.gfft_lanes, k.stream), "group fft kernels"); rc != H2_OK) return rc;
  return A.release();
}

int h2_fft_group(h2_curve_t curve, uint64_t* points_jac, const uint64_t omega[4], uint32_t log_n) {
  std::lock_guard<std::recursive_mutex> lk(g_h2_mu);
  if (!g_h2.ready) return H2_ENOTINIT;
  if (!curve_ok((int)curve) || !points_jac || !omega || log_n > 26) return H2_EINVAL;
  if (log_n == 0) return H2_OK;
  DevCtx& c = g_h2.ctx[0];
  DeviceGuard dg(c.device);
  const size_t bytes = ((size_t)96) << log_n;
  ArenaLease stage(c.stage, bytes, c.stream);
  if (stage.rc != H2_OK) return stage.rc;
  H2_TRY(hipMemcpyAsync(c.stage.p, points_jac, bytes, hipMemcpyHostToDevice, c.stream));
  int rc = h2_fft_group_device(curve, c.stage.p, omega, log_n, c.stream);
  if (rc != H2_OK) return rc;
  H2_TRY(hipMemcpyAsync(points_jac, c.stage.p, bytes, hipMemcpyDeviceToHost, c.stream));
  return stage.wait();
}

// ParamsKZG's g_to_lagrange: the transform above on affine points, scaled and normalised (h2_group_fft.hpp)
int h2_g_to_lagrange_device(h2_curve_t curve, const void* d_g_affine, uint32_t log_n, const uint64_t omega_inv[4],
                            const uint64_t scale[4], void* d_out_affine, void* stream_) {
  Call k(stream_);
  if (k.rc != H2_OK) return k.rc;
  if (!curve_ok((int)curve) || !d_g_affine || !d_out_affine || !omega_inv || !scale || log_n > 26) return H2_EINVAL;
  const uintptr_t in = (uintptr_t)d_g_affine, out = (uintptr_t)d_out_affine, bytes = (uintptr_t)64 << log_n;
  if ((in & 15) || (out & 15)) return H2_EINVAL;
  if (in != out && in < out + bytes && out < in + bytes) return H2_EINVAL;      // a partial overlap
  const CurveOps* ops = ops_of((int)curve);
  ArenaLease A(k.c->msm_ws.of(k.stream), ops->group_fft_scratch(log_n), k.stream);      // the MSM workspace, idle here
  if (A.rc != H2_OK) return A.rc;
  if (int rc = launched(ops->g_to_lagrange(d_g_affine, d_out_affine, A.a.p, omega_inv, scale, log_n, g_knobs.gfft_lanes, k.stream),
                        "g_to_lagrange kernels");
      rc != H2_OK)
    return rc;
  return A.release();
}

int h2_g_to_lagrange(h2_curve_t curve, const uint64_t* g_affine, uint32_t log_n, const uint64_t omega_inv[4],
                     const uint64_t scale[4], uint64_t* out_affine) {
  std::lock_guard<std::recursive_mutex> lk(g_h2_mu);
  if (!g_h2.ready) return H2_ENOTINIT;
  if (!curve_ok((int)curve) || !g_affine || !out_affine || !omega_inv || !scale || log_n > 26) return H2_EINVAL;
  DevCtx& c = g_h2.ctx[0];
  DeviceGuard dg(c.device);
  const size_t bytes = ((size_t)64) << log_n;
  ArenaLease stage(c.stage, bytes, c.stream);
  if (stage.rc != H2_OK) return stage.rc;
  H2_TRY(hipMemcpyAsync(c.stage.p, g_affine, bytes, hipMemcpyHostToDevice, c.stream));
  int rc = h2_g_to_lagrange_device(curve, c.stage.p, log_n, omega_inv, scale, c.stage.p, c.stream);
  if (rc != H2_OK) return rc;
  H2_TRY(hipMemcpyAsync(out_affine, c.stage.p, bytes, hipMemcpyDeviceToHost, c.stream));
  return stage.wait();
}

int h2_ntt(h2_curve_t curve, uint64_t* a, const uint64_t omega[4], uint32_t log_n) {
  uint64_t* cols[1] = {a};
  return h2_ntt_batch(curve, cols, 1, omega, log_n);
}

}  // extern "C"
