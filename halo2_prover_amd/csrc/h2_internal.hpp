// h2_internal.hpp -- state shared by the translation units behind the C ABI (h2_capi.hip, h2_selftest.hip, the C++ prover).
//
// One DevCtx per GPU the process drives (h2_init: one; h2_init_devices: several).  Every scratch arena remembers the
// stream that used it last and an event recorded behind that use, so a call on ANOTHER stream first waits for it:
// callers may hand any stream to the *_device entry points (include/h2hip.h, threading paragraph).  The MSM and the
// NTT have separate arenas, so an MSM on one stream and an NTT on another do overlap.
#pragma once
#include <hip/hip_runtime.h>

#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/h2hip.h"
#include "h2_curve_ops.hpp"
#include "h2_msm.hpp"
#include "h2_poseidon_ops.hpp"

namespace h2 {

struct Arena {
  void* p = nullptr;
  size_t bytes = 0;
  hipEvent_t ev = nullptr;        // recorded after the last enqueue that used the arena
  hipStream_t last = nullptr;
  bool used = false;
  // MSM workspace: [clean_off, clean_off + clean_bytes) is zero when the work enqueued so far has run -- the previous MSM
  // launch sequence zeroed its counter region again on its way out (msm_rowcol_kernel) -- so the next one skips its memset.
  // Each ArenaLease hands this to its user and clears it; an MSM sets it again once its launch sequence is enqueued whole
  size_t clean_off = 0, clean_bytes = 0;
};

// Scratch that a launch sequence owns from its first kernel to its last (the MSM workspace, the NTT's second buffer): one
// arena per stream for up to H2_ARENA_SLOTS streams, so that launch sequences enqueued on different streams run side by
// side (two proofs in flight on one GPU: bench.py's `two_steps_in_flight`).  A further stream takes over the slot that
// has been idle longest; its ArenaLease orders it behind that slot's previous user (an event wait), as it ordered every
// stream behind every other before round 3.
constexpr int H2_ARENA_SLOTS = 4;
struct ArenaSet {
  Arena slot[H2_ARENA_SLOTS];
  hipStream_t owner[H2_ARENA_SLOTS] = {};
  bool owned[H2_ARENA_SLOTS] = {};
  uint64_t used_at[H2_ARENA_SLOTS] = {};
  uint64_t clock = 0, takeovers = 0;
  Arena& of(hipStream_t s) {
    int pick = -1;
    for (int i = 0; i < H2_ARENA_SLOTS && pick < 0; i++)
      if (owned[i] && owner[i] == s) pick = i;
    for (int i = 0; i < H2_ARENA_SLOTS && pick < 0; i++)
      if (!owned[i]) pick = i;
    if (pick < 0) {
      pick = 0;
      for (int i = 1; i < H2_ARENA_SLOTS; i++)
        if (used_at[i] < used_at[pick]) pick = i;
      takeovers++;
    }
    owned[pick] = true;
    owner[pick] = s;
    used_at[pick] = ++clock;
    return slot[pick];
  }
};

struct TwiddleEntry {
  int field;
  uint32_t log_n;
  uint64_t omega[4];
  bool scaled;            // the inter-pass twiddles carry `scale` (a two-pass scaled transform)
  uint64_t scale[4];
  void* tw;
  uint64_t stamp;
};

// the constants of one Poseidon instance (h2_poseidon.hpp) in HBM, in the kernels' working form
struct PoseidonTable {
  int field;
  uint32_t width;      // 3: the dense part alone; 5, 9: dense and sparse part (h2_poseidon.hpp: poseidon_table_elems)
  uint32_t r_f, r_p;
  void* d;
};

struct DevCtx {
  int device = -1;
  hipStream_t stream = nullptr;   // the library's own (blocking) stream on this device
  hipStream_t side_stream = nullptr;   // the C++ prover's second stream (transforms beside the MSM tails), created on demand
  hipEvent_t side_ev[3] = {nullptr, nullptr, nullptr};
  ArenaSet msm_ws, ntt_ws;
  Arena stage, div_ws;
  hipEvent_t shard_ev = nullptr;     // C++ prover: this context's share of a commit phase is done / the columns are final
  hipEvent_t tail_event = nullptr;   // recorded behind the accumulate kernel of the latest MSM (h2_stream_wait_msm_tail)
  hipEvent_t tail_wait = nullptr;    // the event to wait on for that: tail_event, or the profiling stop event of the
                                     // launch when profiling records one at the same place (an event record costs ~6 us
                                     // of stream time: profiles/r03 step timeline)
  bool tail_recorded = false, tail_wanted = false;   // the event costs ~5 us per MSM: recorded once somebody asked
  std::vector<TwiddleEntry> twiddles;
  uint64_t stamp = 0;
  std::vector<PoseidonTable> poseidon_tables;   // at most POSEIDON_TABLE_SLOTS, oldest first (poseidon_table_get)
  // kernel timing for the roofline (h2_profile_*): event pairs around the bucket-accumulate kernel
  std::vector<std::pair<hipEvent_t, hipEvent_t>> prof_events;
  size_t prof_used = 0;
  double prof_alg_bytes = 0;
};

struct BasesEntry {
  int curve;
  size_t n;
  MsmGeom geom;
  std::vector<void*> table;       // per context: W * n affine points in the working form
  size_t table_bytes;
};

// a program compiled by h2_expr_compile (h2_expr_program.hpp): host state only until a context first evaluates it
struct ExprEntry {
  int curve;
  h2_expr_info_t info;
  std::vector<uint32_t> code;         // three words per instruction (pk::XInstr)
  std::vector<uint64_t> table;        // the constant table in the kernel's working form, 4 limbs each; variables zero
  std::vector<uint32_t> var_slot;     // table index of each variable
  std::vector<uint8_t> dump;          // what h2_expr_dump reports
  std::vector<void*> d_code;          // per context: the code in HBM, uploaded by the context's first eval
};

struct Global {
  bool ready = false;
  std::vector<DevCtx> ctx;
  std::map<uint64_t, BasesEntry> bases;
  std::map<uint64_t, ExprEntry> exprs;
  uint64_t next_handle = 1;
  bool profiling = false;
  std::string last_error;
};

extern Global g_h2;
extern std::recursive_mutex g_h2_mu;

// Test-only state, moved by the hooks of include/h2hip_selftest.h (h2_selftest.hip) alone: the defaults are the product's
struct TestKnobs {
  uint64_t msm_max_entries = (1ull << 31) - 1;   // entries one sort launch may hold (msm_cols_per_launch)
  // guard mode: the MSM workspace is laid out with a red zone behind every region, filled with a pattern before each
  // launch sequence and inspected after it; poke: one byte behind the second region is written first, to test the checker
  bool msm_guard = false, msm_guard_poke = false;
  bool sort2_pack = true;                        // false: the unpacked forms of the two-level sort and the staged scatter
  size_t points_small_max = MSM_POINTS_SMALL_MAX;   // terms below which h2_msm_points* takes the double-and-add route
  int gfft_lanes = 0;                            // lanes per butterfly of the group FFT: 0 = by size, 1, 4
  uint32_t poseidon_merkle_tail = 0;             // nodes a Merkle level may have to be finished by the tail launch; 0: the default
  int poseidon_form = 0;                         // the hash kernel's products: 0 = by size, 1 = the compiler's form, 2 = single-chain
  int poseidon_wide_form = 0;                    // the wide permutation kernel's partial rounds: 0 = the width's own, 1 = dense, 2 = sparse
  int poseidon_walk_form = 0;                    // the Merkle walker and update: 0 = by size, 1 = a lane per hash, 2 = a quad per hash
  int ipa_inv_form = 0;                          // the IPA prover's transcript step inverts by: 0 = divsteps, 1 = fe_inv's Fermat chain
};
struct TestCounters {
  uint64_t guard_launches = 0, guard_violations = 0;
  std::string guard_first;
  uint64_t arena_growths = 0, arena_waits = 0;
};
extern TestKnobs g_knobs;
extern TestCounters g_counts;

// the process's current HIP device is switched for the lifetime of the guard
struct DeviceGuard {
  int prev = -1;
  bool switched = false;
  explicit DeviceGuard(int device) {
    if (hipGetDevice(&prev) == hipSuccess && prev != device) switched = hipSetDevice(device) == hipSuccess;
  }
  ~DeviceGuard() {
    if (switched) (void)hipSetDevice(prev);
  }
};

int dev_fail(hipError_t e, const char* where);
// the status of a launch (sequence) named `what`
inline int launched(hipError_t e, const char* what) { return e == hipSuccess ? H2_OK : dev_fail(e, what); }
const CurveOps* ops_of(int curve);
const PoseidonOps* poseidon_ops_of(int curve);
bool curve_ok(int c);
// context of the calling thread's current HIP device (the only context when there is just one); null if none
DevCtx* ctx_current();
size_t ctx_index(const DevCtx* c);

// hipMalloc of the buffer named `what`: H2_ENOMEM (sticky error cleared, last_error set, *p = null) if it fails
int device_alloc(void** p, size_t bytes, const char* what);
// The Poseidon table of (curve, width 3 | 5 | 9, r_f, r_p) as Montgomery limbs (host): the dense part, h2_poseidon_wide_
// constants' elements, and with `sparse` (widths 5, 9) the sparse part behind it (h2_poseidon.hpp: poseidon_table_elems in all).
// ConstantLength<len>'s capacity word len 2^64.  False when the partial rounds do not factor (h2_poseidon_host.hpp)
bool poseidon_wide_table_mont(int curve, uint32_t width, uint32_t r_f, uint32_t r_p, bool sparse, uint64_t* out);
void poseidon_capacity_mont(int curve, uint64_t len, uint64_t out[4]);
// scratch device memory owned by one call: freed on every way out of it
struct HipFree { void operator()(void* p) const { (void)hipFree(p); } };
using DeviceBuffer = std::unique_ptr<void, HipFree>;

// One use of an arena by the work a call enqueues on `s`.  The constructor grows the arena if needed and orders `s`
// behind the previous user on another stream (status in rc); release() records the arena's event behind this use, the
// event the next user on another stream waits on; wait() synchronises `s` instead, after which the arena is idle and
// needs no event.  A lease ended neither way -- an error path, or a user with no status to report -- records the event
// in its destructor, result ignored, so that work already enqueued is still waited for.
struct ArenaLease {
  Arena& a;
  hipStream_t s;
  size_t clean_bytes = 0;   // a.clean_bytes as the previous user left it
  int rc;
  ArenaLease(Arena& arena, size_t want, hipStream_t stream);
  ArenaLease(const ArenaLease&) = delete;
  ~ArenaLease() noexcept;
  int release();
  int wait();
 private:
  bool released = false;
  int acquire(size_t want);
};

// enqueue m MSMs (columns of n scalars, col_stride elements apart, bases first_base ... first_base + n - 1 of the
// registered vector) -> m Jacobian (96 B) or affine (64 B) points at d_out; all on `stream`
// `per_column` (optional, m <= MSM_MAX_MULTI entries of the same length as `be`): column j commits against
// per_column[j] instead of `be` -- the columns of one launch may use different bases
int msm_device_run(DevCtx& c, int curve, const BasesEntry& be, const void* d_scalars, size_t first_base, size_t n,
                   size_t col_stride, size_t m, void* d_out, bool affine_out, hipStream_t stream,
                   const BasesEntry* const* per_column = nullptr);
// columns of n scalars one MSM launch sequence takes under this geometry (0: a single column is already too long); a wider
// call runs in groups of that many, and columns with their own bases (per_column) must fit one group
size_t msm_cols_per_launch(const MsmGeom& geom, size_t n);
// The next launch sequence of a call with m columns left: the columns it takes (0: a single column is already too long),
// its workspace, and the bounds proof of every kernel's index range against the region it indexes (null, or the violated
// condition).  msm_device_run / the table-free route launch what these return; the host-only hooks report it
// (proved against the layout's own size, ws.total; msm_run_group holds the leased arena's real size against that)
struct MsmGroupPlan {
  size_t cols;
  MsmWorkspace ws;
  const char* broken;
};
// (n_bases is the REGISTERED length whatever the range: a sorted entry is w * n_bases + i relative to the table row of the first base)
inline MsmGroupPlan msm_plan_group(const MsmGeom& g, size_t n_bases, size_t n, size_t m, size_t col_stride, bool guard, bool pack) {
  MsmGroupPlan p{};
  p.cols = std::min(m, msm_cols_per_launch(g, n));
  if (p.cols == 0) return p;
  p.ws = msm_workspace(n, p.cols, g, guard ? 256u : 0u, n_bases, pack);
  p.broken = msm_check(p.ws, g, n, p.cols, col_stride, (uint32_t)n_bases, p.ws.total);
  return p;
}
inline MsmGroupPlan msm_points_plan_group(const MsmGeom& g, size_t n, size_t m, size_t col_stride, bool guard) {
  MsmGroupPlan p{};
  p.cols = std::min(m, msm_points_cols_per_launch(g, n));
  if (p.cols == 0) return p;
  p.ws = msm_points_workspace(n, p.cols, g, guard ? 256u : 0u);
  p.broken = msm_points_check(p.ws, g, n, p.cols, col_stride, p.ws.total);
  return p;
}
int ntt_enqueue(DevCtx& c, int curve, void* d_a, size_t m, const uint64_t omega[4], uint32_t log_n, hipStream_t stream,
                const uint64_t* scale = nullptr);
// EvaluationDomain::coeff_to_extended (h2_coeff_to_extended_device; arguments checked by the caller, ext_log_n >= 1):
// the tables of (ext_omega, ext_log_n) unscaled -- ntt_enqueue's entry -- and its second buffer on `stream`
int coeff_to_extended_enqueue(DevCtx& c, int curve, const void* d_coeff, size_t col_stride, uint32_t log_n, size_t m,
                              const uint64_t zeta[4], const uint64_t ext_omega[4], uint32_t ext_log_n, void* d_out,
                              hipStream_t stream);
// eval_polynomial (h2_poly_eval_device; arguments checked by the caller, n >= 1, q >= 1): q jobs in groups of at most
// 65535, the job table and the groups' scratch (h2_poly.hpp) in c.div_ws for the length of the call.  d_polys and
// points are host arrays, read before the call returns
int poly_eval_enqueue(DevCtx& c, int curve, const void* const* d_polys, size_t n, const uint64_t* points, size_t q, void* d_out,
                      hipStream_t stream);
// EvaluationDomain::extended_to_coeff, with divide_by_vanishing_poly when d_t is set (h2_extended_to_coeff_device;
// arguments checked by the caller): ntt_enqueue's table for (ext_omega_inv, ext_log_n, scale) and its second buffer
int extended_to_coeff_enqueue(DevCtx& c, int curve, const void* d_ext, uint32_t ext_log_n, size_t m,
                              const uint64_t ext_omega_inv[4], const uint64_t scale[4], const uint64_t zeta_inv[4], const void* d_t,
                              size_t t_period, void* d_out, size_t out_len, size_t out_stride, hipStream_t stream);
// permutation::Argument::commit's grand products (h2_permutation_product_device; pointers, alignment and overlap checked by
// the caller, n_cols >= 1, chunk_len >= 1, m >= 1): every launch bound proven first (H2_EDEVICE and last_error otherwise),
// the tables (h2_permutation.hpp) in one upload and the scan values in c.div_ws for the length of the call.  d_values,
// d_sigma, beta and gamma are host arrays, read before the call returns
int permutation_product_enqueue(DevCtx& c, int curve, const void* const* d_values, const void* const* d_sigma, size_t n_cols,
                                size_t chunk_len, size_t u, size_t m, const uint64_t* beta, const uint64_t* gamma, const uint64_t omega[4],
                                const uint64_t delta[4], void* d_z, size_t col_stride, hipStream_t stream);
int msm_common_checks(int curve, uint64_t handle, size_t first, size_t n, size_t m, const BasesEntry** be);

#define H2_TRY(call)                                        \
  do {                                                      \
    hipError_t _e = (call);                                 \
    if (_e != hipSuccess) return ::h2::dev_fail(_e, #call); \
  } while (0)

}  // namespace h2
