// h2_lookup.hpp -- the lookup argument's two data-dependent steps over resident columns of the scalar field:
// permute_expression_pair (halo2_proofs @6b43b6b src/plonk/lookup/prover.rs; the loop is restated in include/h2hip.h and
// DESIGN.md 7.9) and the per-row ratio of commit_product, whose running product is poly_scan mode 1 (h2_poly.hpp).
//
// The order of field elements is that of their canonical integers, so every column is de-Montgomerised once into 8 x u32
// keys and sorted by an LSD radix sort of 8-bit digits.  Sort job j < mm is the input column of lookup j, job mm + j its
// table column; grid.y = job everywhere.
//   prep     key = fe_from_mont(column) -> keys0; AND and OR of all keys of the job (wave shuffles, then 16 integer
//            atomics per workgroup).  A byte on which AND and OR agree is constant over the column: its pass is skipped.
//   plan     per job the mask of the up to 32 non-constant digits and their number, in device memory.  The host never
//            reads it: all 32 passes are enqueued and pass k of a job with fewer than k + 1 digits returns at once, so the
//            call stays asynchronous.  Pass k reads keys[k & 1] and writes keys[(k + 1) & 1].
//   pass k   hist (per tile of LOOKUP_TILE rows the count of each digit value, digit-major: hist[value][tile]), scan (one
//            workgroup per job: exclusive prefix over the 256 * tiles counts), scatter (stable: ranks among equal digits
//            by wave ballots and a per-wave count table, the tile staged in LDS in digit order, stored so that lane j
//            holds staged key j: the keys of one digit value leave as one run).
//   assign   flags of first occurrences in the sorted input; each first occurrence binary-searches the sorted table and
//            marks the first instance of its value removed (distinct values: distinct marks) or raises the status word;
//            per-tile counts of repeated rows and of surviving table entries, one scan of both over the tiles, the
//            repeated rows compacted by rank, and survivor j stored to the repeated row of rank R - 1 - j.  Outputs are
//            re-Montgomerised on the way out (one product per element).
// Every index is formed from usable_rows, the tile and job numbers, a digit value below 256 and ranks that are guarded
// against usable_rows before they address anything: a column that is not canonical changes the order, never the range.
#pragma once
#include "h2_curve_ops.hpp"
#include "h2_field.hpp"

#include <cstring>

namespace h2 {

constexpr uint32_t LOOKUP_TILE = 1024;            // rows per workgroup and sort pass = threads per workgroup
constexpr uint32_t LOOKUP_WAVES = LOOKUP_TILE / 64;
constexpr size_t LOOKUP_MAX_ROWS = (size_t)1 << 26;
constexpr size_t LOOKUP_WS_CAP = (size_t)1 << 30;  // scratch of one group of lookups (always at least one lookup)
constexpr size_t LOOKUP_MAX_CELLS = (size_t)1 << 57;   // m * col_stride: byte ranges stay below 2^63
constexpr uint32_t LOOKUP_MAX_JOBS = 65534;       // grid.y
constexpr int LOOKUP_RUN = 4;                     // rows per thread of the ratio kernel: one inversion per run

// scratch of one group of mm lookups of u rows (offsets in bytes from a 256-byte aligned base)
struct LookupWorkspace {
  uint32_t u, tiles, mm, jobs;
  size_t off_keys0, off_keys1;     // jobs * u keys of 32 bytes each
  size_t off_hist;                 // jobs * 256 * tiles words
  size_t off_and;                  // jobs * 8 words, preset to ~0
  size_t off_or;                   // jobs * 8 words      -- [off_or, off_or + zero_bytes) is preset to zero
  size_t off_removed;              // mm * u bytes
  size_t zero_bytes;
  size_t off_plan;                 // jobs * 2 words: digit mask, number of passes
  size_t off_isrep;                // mm * u bytes
  size_t off_repcnt, off_survcnt;  // mm * (tiles + 1) words each
  size_t off_reprow;               // mm * u words
  size_t total;
};

inline size_t lookup_align(size_t x) { return (x + 255) & ~(size_t)255; }

inline LookupWorkspace lookup_workspace(size_t u, size_t mm) {
  LookupWorkspace w{};
  w.u = (uint32_t)u;
  w.tiles = (uint32_t)((u + LOOKUP_TILE - 1) / LOOKUP_TILE);
  w.mm = (uint32_t)mm;
  w.jobs = (uint32_t)(2 * mm);
  size_t o = 0;
  auto take = [&](size_t bytes) {
    const size_t at = o;
    o += lookup_align(bytes);
    return at;
  };
  w.off_keys0 = take((size_t)w.jobs * u * 32);
  w.off_keys1 = take((size_t)w.jobs * u * 32);
  w.off_hist = take((size_t)w.jobs * 256 * w.tiles * 4);
  w.off_and = take((size_t)w.jobs * 32);
  w.off_or = take((size_t)w.jobs * 32);
  w.off_removed = take(mm * u);
  w.zero_bytes = o - w.off_or;
  w.off_plan = take((size_t)w.jobs * 8);
  w.off_isrep = take(mm * u);
  w.off_repcnt = take(mm * ((size_t)w.tiles + 1) * 4);
  w.off_survcnt = take(mm * ((size_t)w.tiles + 1) * 4);
  w.off_reprow = take(mm * u * 4);
  w.total = o;
  return w;
}

// lookups of u rows one launch sequence takes: grid.y and the scratch cap
inline size_t lookup_group(size_t u, size_t m) {
  const size_t per = lookup_workspace(u, 1).total;
  size_t g = LOOKUP_WS_CAP / per;
  if (g < 1) g = 1;
  if (g > LOOKUP_MAX_JOBS / 2) g = LOOKUP_MAX_JOBS / 2;
  return g < m ? g : m;
}

// The bounds every kernel below relies on, proven on the host before anything is enqueued (in the style of msm_check):
// null, or the violated condition
inline const char* lookup_check(const LookupWorkspace& w, size_t u, size_t mm, size_t col_stride, size_t arena_bytes) {
#define H2_LOOKUP_REQUIRE(cond) \
  if (!(cond)) return #cond
  H2_LOOKUP_REQUIRE(u >= 1 && u <= LOOKUP_MAX_ROWS);
  H2_LOOKUP_REQUIRE(mm >= 1 && 2 * mm <= LOOKUP_MAX_JOBS);
  H2_LOOKUP_REQUIRE(w.u == u && w.mm == mm && w.jobs == 2 * mm);
  H2_LOOKUP_REQUIRE(col_stride >= u);
  H2_LOOKUP_REQUIRE((size_t)w.tiles * LOOKUP_TILE >= u && ((size_t)w.tiles - 1) * LOOKUP_TILE < u);   // row = tile * T + thread covers [0, u)
  // each region holds what its kernels index: row < u, job < jobs, lookup < mm, digit value < 256, tile <= tiles
  H2_LOOKUP_REQUIRE(w.off_keys0 + (size_t)w.jobs * u * 32 <= w.off_keys1);
  H2_LOOKUP_REQUIRE(w.off_keys1 + (size_t)w.jobs * u * 32 <= w.off_hist);
  H2_LOOKUP_REQUIRE((uint64_t)256 * w.tiles <= 0xFFFFFFFFull);                                         // the scan's 32-bit entry index
  H2_LOOKUP_REQUIRE(w.off_hist + (size_t)w.jobs * 256 * w.tiles * 4 <= w.off_and);
  H2_LOOKUP_REQUIRE(w.off_and + (size_t)w.jobs * 32 <= w.off_or);
  H2_LOOKUP_REQUIRE(w.off_or + (size_t)w.jobs * 32 <= w.off_removed);
  H2_LOOKUP_REQUIRE(w.off_removed + mm * u <= w.off_plan && w.off_or + w.zero_bytes <= w.off_plan);
  H2_LOOKUP_REQUIRE(w.off_plan + (size_t)w.jobs * 8 <= w.off_isrep);
  H2_LOOKUP_REQUIRE(w.off_isrep + mm * u <= w.off_repcnt);
  H2_LOOKUP_REQUIRE(w.off_repcnt + mm * ((size_t)w.tiles + 1) * 4 <= w.off_survcnt);
  H2_LOOKUP_REQUIRE(w.off_survcnt + mm * ((size_t)w.tiles + 1) * 4 <= w.off_reprow);
  H2_LOOKUP_REQUIRE(w.off_reprow + mm * u * 4 <= w.total);
  H2_LOOKUP_REQUIRE((w.off_keys0 & 255) == 0 && (w.off_keys1 & 255) == 0);
  H2_LOOKUP_REQUIRE(w.total <= arena_bytes);
#undef H2_LOOKUP_REQUIRE
  return nullptr;
}

// canonical key: 8 x u32, little-endian words; byte p (0 = least significant) is sort digit p
struct LookupKey {
  uint32_t v[8];
};
__device__ __forceinline__ LookupKey lookup_key_load(const U128* p) {
  const U128 lo = p[0], hi = p[1];
  return LookupKey{{lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w}};
}
__device__ __forceinline__ void lookup_key_store(U128* p, const LookupKey& k) {
  p[0] = U128{k.v[0], k.v[1], k.v[2], k.v[3]};
  p[1] = U128{k.v[4], k.v[5], k.v[6], k.v[7]};
}
__device__ __forceinline__ bool lookup_key_lt(const LookupKey& a, const LookupKey& b) {
  bool lt = false;
#pragma unroll
  for (int i = 0; i < 8; i++) lt = a.v[i] < b.v[i] || (a.v[i] == b.v[i] && lt);     // the highest differing word decides
  return lt;
}
__device__ __forceinline__ bool lookup_key_eq(const LookupKey& a, const LookupKey& b) {
  uint32_t o = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) o |= a.v[i] ^ b.v[i];
  return o == 0;
}
__device__ __forceinline__ uint32_t lookup_digit(const LookupKey& k, uint32_t p) {
  uint32_t w = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) w = (p >> 2) == (uint32_t)i ? k.v[i] : w;
  return (w >> (8 * (p & 3))) & 255u;
}
// digit index of pass k: the k-th set bit of the job's mask (k < popcount(mask))
__device__ __forceinline__ uint32_t lookup_pass_digit(uint32_t mask, uint32_t k) {
  for (uint32_t t = 0; t < k; t++) mask &= mask - 1;
  return (uint32_t)__ffs(mask) - 1;
}
// exclusive rank of a flag among the LOOKUP_TILE threads of the workgroup, and the number of flags set; wsum: LOOKUP_WAVES words of LDS
__device__ __forceinline__ uint32_t lookup_block_rank(bool f, uint32_t* wsum, uint32_t& total) {
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t bal = __ballot(f);
  if (lane == 0) wsum[wave] = (uint32_t)__popcll(bal);
  __syncthreads();
  uint32_t base = 0, all = 0;
#pragma unroll
  for (uint32_t w = 0; w < LOOKUP_WAVES; w++) {
    const uint32_t c = wsum[w];
    base += w < wave ? c : 0;
    all += c;
  }
  total = all;
  return base + (uint32_t)__popcll(bal & (((uint64_t)1 << lane) - 1));
}

// ---- prep: grid (tiles, jobs) -----------------------------------------------------------------------------------------
template <class FP>
__global__ void __launch_bounds__(LOOKUP_TILE)
lookup_prep_kernel(const U128* __restrict__ input, const U128* __restrict__ table, size_t col_stride, uint32_t u, uint32_t mm,
                   U128* __restrict__ keys0, uint32_t* __restrict__ and_words, uint32_t* __restrict__ or_words) {
  __shared__ uint32_t red[16];
  const uint32_t job = blockIdx.y, i = blockIdx.x * LOOKUP_TILE + threadIdx.x;
  const U128* col = (job < mm ? input + 2 * col_stride * job : table + 2 * col_stride * (job - mm));
  if (threadIdx.x < 16) red[threadIdx.x] = threadIdx.x < 8 ? 0xFFFFFFFFu : 0u;
  __syncthreads();
  uint32_t a[8], o[8];
#pragma unroll
  for (int w = 0; w < 8; w++) {
    a[w] = 0xFFFFFFFFu;
    o[w] = 0;
  }
  if (i < u) {
    const Fe<FP> x = fe_from_mont(fe_load<FP>(col + 2 * (size_t)i));
    fe_store<FP>(keys0 + 2 * ((size_t)job * u + i), x);
#pragma unroll
    for (int w = 0; w < 8; w++) a[w] = o[w] = x.v[w];
  }
#pragma unroll
  for (int w = 0; w < 8; w++)
    for (int d = 32; d >= 1; d >>= 1) {
      a[w] &= (uint32_t)__shfl_xor((int)a[w], d);
      o[w] |= (uint32_t)__shfl_xor((int)o[w], d);
    }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int w = 0; w < 8; w++) {
      atomicAnd(&red[w], a[w]);
      atomicOr(&red[8 + w], o[w]);
    }
  }
  __syncthreads();
  if (threadIdx.x < 8) atomicAnd(&and_words[8 * job + threadIdx.x], red[threadIdx.x]);
  else if (threadIdx.x < 16) atomicOr(&or_words[8 * job + threadIdx.x - 8], red[threadIdx.x]);
}

// ---- plan: grid (jobs), 64 threads ------------------------------------------------------------------------------------
static __global__ void __launch_bounds__(64)
lookup_plan_kernel(const uint32_t* __restrict__ and_words, const uint32_t* __restrict__ or_words, uint32_t* __restrict__ plan) {
  const uint32_t job = blockIdx.x, p = threadIdx.x;
  bool active = false;
  if (p < 32) {
    const uint32_t a = (and_words[8 * job + (p >> 2)] >> (8 * (p & 3))) & 255u;
    const uint32_t o = (or_words[8 * job + (p >> 2)] >> (8 * (p & 3))) & 255u;
    active = a != o;
  }
  const uint32_t mask = (uint32_t)__ballot(active);
  if (p == 0) {
    plan[2 * job] = mask;
    plan[2 * job + 1] = (uint32_t)__popc(mask);
  }
}

// ---- pass k, hist: grid (tiles, jobs) ---------------------------------------------------------------------------------
static __global__ void __launch_bounds__(LOOKUP_TILE)
lookup_hist_kernel(const U128* __restrict__ keys0, const U128* __restrict__ keys1, const uint32_t* __restrict__ plan,
                   uint32_t* __restrict__ hist, uint32_t u, uint32_t tiles, uint32_t k) {
  __shared__ uint32_t cnt[256];
  const uint32_t job = blockIdx.y, tile = blockIdx.x;
  if (k >= plan[2 * job + 1]) return;
  const uint32_t p = lookup_pass_digit(plan[2 * job], k);
  const uint32_t* src = (const uint32_t*)((k & 1) ? keys1 : keys0) + 8 * (size_t)job * u;
  if (threadIdx.x < 256) cnt[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t i = tile * LOOKUP_TILE + threadIdx.x;
  if (i < u) atomicAdd(&cnt[(src[8 * (size_t)i + (p >> 2)] >> (8 * (p & 3))) & 255u], 1u);
  __syncthreads();
  if (threadIdx.x < 256) hist[((size_t)job * 256 + threadIdx.x) * tiles + tile] = cnt[threadIdx.x];
}

// in-place exclusive prefix of a[0 .. n) by one workgroup of LOOKUP_TILE threads; the sum goes to *total when set
__device__ __forceinline__ void lookup_block_scan(uint32_t* __restrict__ a, uint32_t n, uint32_t* total) {
  __shared__ uint32_t wsum[LOOKUP_WAVES];
  const uint32_t per = (n + LOOKUP_TILE - 1) / LOOKUP_TILE;
  const uint64_t lo64 = (uint64_t)threadIdx.x * per;
  const uint32_t lo = lo64 < n ? (uint32_t)lo64 : n, hi = lo64 + per < n ? (uint32_t)(lo64 + per) : n;
  uint32_t sum = 0;
  for (uint32_t t = lo; t < hi; t++) sum += a[t];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t inc = sum;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t up = (uint32_t)__shfl_up((int)inc, d);
    if (lane >= (uint32_t)d) inc += up;
  }
  if (lane == 63) wsum[wave] = inc;
  __syncthreads();
  uint32_t base = 0, all = 0;
#pragma unroll
  for (uint32_t w = 0; w < LOOKUP_WAVES; w++) {
    const uint32_t c = wsum[w];
    base += w < wave ? c : 0;
    all += c;
  }
  uint32_t run = base + inc - sum;
  for (uint32_t t = lo; t < hi; t++) {
    const uint32_t c = a[t];
    a[t] = run;
    run += c;
  }
  if (total && threadIdx.x == 0) *total = all;
}

// ---- pass k, scan: grid (jobs) ----------------------------------------------------------------------------------------
static __global__ void __launch_bounds__(LOOKUP_TILE)
lookup_scan_kernel(const uint32_t* __restrict__ plan, uint32_t* __restrict__ hist, uint32_t tiles, uint32_t k) {
  const uint32_t job = blockIdx.x;
  if (k >= plan[2 * job + 1]) return;
  lookup_block_scan(hist + (size_t)job * 256 * tiles, 256 * tiles, nullptr);
}

// ---- pass k, scatter: grid (tiles, jobs) ------------------------------------------------------------------------------
static __global__ void __launch_bounds__(LOOKUP_TILE)
lookup_scatter_kernel(U128* __restrict__ keys0, U128* __restrict__ keys1, const uint32_t* __restrict__ plan,
                      const uint32_t* __restrict__ hist, uint32_t u, uint32_t tiles, uint32_t k) {
  __shared__ uint32_t cnt[LOOKUP_WAVES][256];     // per wave and digit value: count, then the count of the earlier waves
  __shared__ uint32_t tot[256];                   // per digit value: count in the tile
  __shared__ uint32_t tstart[256];                // exclusive prefix of tot: where the value's run starts in the stage
  __shared__ U128 stage[2 * LOOKUP_TILE];
  const uint32_t job = blockIdx.y, tile = blockIdx.x;
  if (k >= plan[2 * job + 1]) return;
  const uint32_t p = lookup_pass_digit(plan[2 * job], k);
  const U128* src = ((k & 1) ? keys1 : keys0) + 2 * (size_t)job * u;
  U128* dst = ((k & 1) ? keys0 : keys1) + 2 * (size_t)job * u;
  for (uint32_t t = threadIdx.x; t < LOOKUP_WAVES * 256; t += LOOKUP_TILE) (&cnt[0][0])[t] = 0;
  __syncthreads();
  const uint32_t first = tile * LOOKUP_TILE, i = first + threadIdx.x;
  const uint32_t nvalid = u - first < LOOKUP_TILE ? u - first : LOOKUP_TILE;
  const bool valid = threadIdx.x < nvalid;
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  LookupKey key{};
  if (valid) key = lookup_key_load(src + 2 * (size_t)i);
  const uint32_t d = valid ? lookup_digit(key, p) : 0u;
  // lanes of this wave that hold the same digit value
  uint64_t peers = __ballot(valid);
#pragma unroll
  for (int b = 0; b < 8; b++) {
    const bool bit = (d >> b) & 1u;
    const uint64_t bal = __ballot(valid && bit);
    peers &= bit ? bal : ~bal;
  }
  const uint32_t rank = (uint32_t)__popcll(peers & (((uint64_t)1 << lane) - 1));
  if (valid && rank == 0) cnt[wave][d] = (uint32_t)__popcll(peers);
  __syncthreads();
  if (threadIdx.x < 256) {
    uint32_t run = 0;
#pragma unroll
    for (uint32_t w = 0; w < LOOKUP_WAVES; w++) {
      const uint32_t c = cnt[w][threadIdx.x];
      cnt[w][threadIdx.x] = run;
      run += c;
    }
    tot[threadIdx.x] = run;
  }
  __syncthreads();
  if (threadIdx.x < 64) {          // one wave: four values per lane
    const uint32_t* from = tot;
    uint32_t* to = tstart;
    const uint32_t c0 = from[4 * lane], c1 = from[4 * lane + 1], c2 = from[4 * lane + 2], c3 = from[4 * lane + 3];
    const uint32_t sum = c0 + c1 + c2 + c3;
    uint32_t inc = sum;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
      const uint32_t up = (uint32_t)__shfl_up((int)inc, s);
      if (lane >= (uint32_t)s) inc += up;
    }
    const uint32_t ex = inc - sum;
    to[4 * lane] = ex;
    to[4 * lane + 1] = ex + c0;
    to[4 * lane + 2] = ex + c0 + c1;
    to[4 * lane + 3] = ex + c0 + c1 + c2;
  }
  __syncthreads();
  if (valid) {
    const uint32_t lp = tstart[d] + cnt[wave][d] + rank;      // < nvalid: a rank among the tile's valid rows
    if (lp < LOOKUP_TILE) lookup_key_store(stage + 2 * lp, key);
  }
  __syncthreads();
  if (valid) {
    const LookupKey k2 = lookup_key_load(stage + 2 * threadIdx.x);
    const uint32_t d2 = lookup_digit(k2, p);
    const uint32_t pos = hist[((size_t)job * 256 + d2) * tiles + tile] + (threadIdx.x - tstart[d2]);
    if (pos < u) lookup_key_store(dst + 2 * (size_t)pos, k2);
  }
}

// ---- assignment -------------------------------------------------------------------------------------------------------
struct LookupAssign {
  const U128* keys0;
  const U128* keys1;
  const uint32_t* plan;
  uint8_t* removed;
  uint8_t* isrep;
  uint32_t* repcnt;
  uint32_t* survcnt;
  uint32_t* reprow;
  U128* out_input;
  U128* out_table;
  uint32_t* status;
  size_t col_stride;
  uint32_t u, tiles, mm;
};
// the sorted keys of a job: where its last pass left them
__device__ __forceinline__ const U128* lookup_sorted(const LookupAssign& A, uint32_t job) {
  return ((A.plan[2 * job + 1] & 1) ? A.keys1 : A.keys0) + 2 * (size_t)job * A.u;
}

// grid (tiles, mm): A' and the first occurrences of S', the marks in the table, the tile's count of repeated rows
template <class FP>
__global__ void __launch_bounds__(LOOKUP_TILE) lookup_flag_kernel(LookupAssign A) {
  __shared__ uint32_t wsum[LOOKUP_WAVES];
  const uint32_t j = blockIdx.y, tile = blockIdx.x, i = tile * LOOKUP_TILE + threadIdx.x, u = A.u;
  const U128* sa = lookup_sorted(A, j);
  const U128* st = lookup_sorted(A, A.mm + j);
  bool rep = false;
  if (i < u) {
    const LookupKey a = lookup_key_load(sa + 2 * (size_t)i);
    const bool first = i == 0 || !lookup_key_eq(a, lookup_key_load(sa + 2 * (size_t)(i - 1)));
    rep = !first;
    Fe<FP> x;
#pragma unroll
    for (int w = 0; w < 8; w++) x.v[w] = a.v[w];
    x = fe_to_mont(x);
    fe_store<FP>(A.out_input + 2 * (A.col_stride * j + i), x);
    A.isrep[(size_t)j * u + i] = rep ? 1 : 0;
    if (first) {
      uint32_t lo = 0, hi = u;                       // lower bound of a in the sorted table: lo <= hi <= u throughout
      while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);  // < hi <= u
        if (lookup_key_lt(lookup_key_load(st + 2 * (size_t)mid), a)) lo = mid + 1;
        else hi = mid;
      }
      if (lo < u && lookup_key_eq(lookup_key_load(st + 2 * (size_t)lo), a)) {
        A.removed[(size_t)j * u + lo] = 1;
        fe_store<FP>(A.out_table + 2 * (A.col_stride * j + i), x);
      } else {
        atomicOr(&A.status[j], 1u);
      }
    }
  }
  uint32_t total;
  (void)lookup_block_rank(rep, wsum, total);
  if (threadIdx.x == 0) A.repcnt[(size_t)j * (A.tiles + 1) + tile] = total;
}

// grid (tiles, mm): the tile's count of table entries that no first occurrence took
static __global__ void __launch_bounds__(LOOKUP_TILE) lookup_survivors_kernel(LookupAssign A) {
  __shared__ uint32_t wsum[LOOKUP_WAVES];
  const uint32_t j = blockIdx.y, tile = blockIdx.x, q = tile * LOOKUP_TILE + threadIdx.x;
  const bool surv = q < A.u && A.removed[(size_t)j * A.u + q] == 0;
  uint32_t total;
  (void)lookup_block_rank(surv, wsum, total);
  if (threadIdx.x == 0) A.survcnt[(size_t)j * (A.tiles + 1) + tile] = total;
}

// grid (mm, 2): exclusive prefix over the tiles of the repeated rows (y = 0) or the survivors (y = 1); entry [tiles] = the sum
static __global__ void __launch_bounds__(LOOKUP_TILE) lookup_tile_scan_kernel(LookupAssign A) {
  uint32_t* a = (blockIdx.y == 0 ? A.repcnt : A.survcnt) + (size_t)blockIdx.x * (A.tiles + 1);
  lookup_block_scan(a, A.tiles, a + A.tiles);
}

// grid (tiles, mm): reprow[rank] = row for the repeated rows, ranks in row order
static __global__ void __launch_bounds__(LOOKUP_TILE) lookup_compact_kernel(LookupAssign A) {
  __shared__ uint32_t wsum[LOOKUP_WAVES];
  const uint32_t j = blockIdx.y, tile = blockIdx.x, i = tile * LOOKUP_TILE + threadIdx.x;
  const bool rep = i < A.u && A.isrep[(size_t)j * A.u + i] != 0;
  uint32_t total;
  const uint32_t rank = A.repcnt[(size_t)j * (A.tiles + 1) + tile] + lookup_block_rank(rep, wsum, total);
  if (rep && rank < A.u) A.reprow[(size_t)j * A.u + rank] = i;
}

// grid (tiles, mm): survivor of rank r (ascending value) -> the repeated row of rank R - 1 - r
template <class FP>
__global__ void __launch_bounds__(LOOKUP_TILE) lookup_fill_kernel(LookupAssign A) {
  __shared__ uint32_t wsum[LOOKUP_WAVES];
  const uint32_t j = blockIdx.y, tile = blockIdx.x, q = tile * LOOKUP_TILE + threadIdx.x, u = A.u;
  const bool surv = q < u && A.removed[(size_t)j * u + q] == 0;
  uint32_t total;
  const uint32_t r = A.survcnt[(size_t)j * (A.tiles + 1) + tile] + lookup_block_rank(surv, wsum, total);
  const uint32_t R = A.repcnt[(size_t)j * (A.tiles + 1) + A.tiles];       // <= u; a failed pair has more survivors than that
  if (surv && r < R) {
    const uint32_t row = A.reprow[(size_t)j * u + (R - 1 - r)];
    if (row < u) {
      const LookupKey t = lookup_key_load(lookup_sorted(A, A.mm + j) + 2 * (size_t)q);
      Fe<FP> x;
#pragma unroll
      for (int w = 0; w < 8; w++) x.v[w] = t.v[w];
      fe_store<FP>(A.out_table + 2 * (A.col_stride * j + row), fe_to_mont(x));
    }
  }
}

// The whole permute of one group of mm lookups on stream s; ws proven by lookup_check.  d_status is zeroed by the caller.
template <class FP>
hipError_t lookup_permute_launch(const void* d_input, const void* d_table, size_t col_stride, const LookupWorkspace& ws, char* base,
                                 void* d_out_input, void* d_out_table, uint32_t* d_status, hipStream_t s) {
  const uint32_t u = ws.u, tiles = ws.tiles, jobs = ws.jobs, mm = ws.mm;
  U128* keys0 = (U128*)(base + ws.off_keys0);
  U128* keys1 = (U128*)(base + ws.off_keys1);
  uint32_t* hist = (uint32_t*)(base + ws.off_hist);
  uint32_t* andw = (uint32_t*)(base + ws.off_and);
  uint32_t* orw = (uint32_t*)(base + ws.off_or);
  uint32_t* plan = (uint32_t*)(base + ws.off_plan);
  hipError_t e = hipMemsetAsync(andw, 0xFF, (size_t)jobs * 32, s);
  if (e != hipSuccess) return e;
  if ((e = hipMemsetAsync(orw, 0, ws.zero_bytes, s)) != hipSuccess) return e;
  const dim3 block(LOOKUP_TILE), by_job(tiles, jobs), by_lookup(tiles, mm);
  hipLaunchKernelGGL(lookup_prep_kernel<FP>, by_job, block, 0, s, (const U128*)d_input, (const U128*)d_table, col_stride, u, mm, keys0,
                     andw, orw);
  hipLaunchKernelGGL(lookup_plan_kernel, dim3(jobs), dim3(64), 0, s, (const uint32_t*)andw, (const uint32_t*)orw, plan);
  for (uint32_t k = 0; k < 32; k++) {
    hipLaunchKernelGGL(lookup_hist_kernel, by_job, block, 0, s, (const U128*)keys0, (const U128*)keys1, (const uint32_t*)plan, hist, u,
                       tiles, k);
    hipLaunchKernelGGL(lookup_scan_kernel, dim3(jobs), block, 0, s, (const uint32_t*)plan, hist, tiles, k);
    hipLaunchKernelGGL(lookup_scatter_kernel, by_job, block, 0, s, keys0, keys1, (const uint32_t*)plan, (const uint32_t*)hist, u, tiles, k);
  }
  LookupAssign A{};
  A.keys0 = keys0;
  A.keys1 = keys1;
  A.plan = plan;
  A.removed = (uint8_t*)(base + ws.off_removed);
  A.isrep = (uint8_t*)(base + ws.off_isrep);
  A.repcnt = (uint32_t*)(base + ws.off_repcnt);
  A.survcnt = (uint32_t*)(base + ws.off_survcnt);
  A.reprow = (uint32_t*)(base + ws.off_reprow);
  A.out_input = (U128*)d_out_input;
  A.out_table = (U128*)d_out_table;
  A.status = d_status;
  A.col_stride = col_stride;
  A.u = u;
  A.tiles = tiles;
  A.mm = mm;
  hipLaunchKernelGGL(lookup_flag_kernel<FP>, by_lookup, block, 0, s, A);
  hipLaunchKernelGGL(lookup_survivors_kernel, by_lookup, block, 0, s, A);
  hipLaunchKernelGGL(lookup_tile_scan_kernel, dim3(mm, 2), block, 0, s, A);
  hipLaunchKernelGGL(lookup_compact_kernel, by_lookup, block, 0, s, A);
  hipLaunchKernelGGL(lookup_fill_kernel<FP>, by_lookup, block, 0, s, A);
  return hipGetLastError();
}

// ---- commit_product's ratio: grid (ceil((u + 1) / (256 * LOOKUP_RUN)), m) ----------------------------------------------
// z[j][i] = (A[i] + beta)(S[i] + gamma) / ((A'[i] + beta)(S'[i] + gamma)) for i < u, one inversion per run of LOOKUP_RUN
// rows; a zero denominator gives 0 for its row alone (batch_invert skips zeros); z[j][u] = 1 so that the scan reads a value
template <class FP>
__global__ void __launch_bounds__(256)
lookup_ratio_kernel(const U128* __restrict__ input, const U128* __restrict__ table, const U128* __restrict__ pin,
                    const U128* __restrict__ ptab, uint32_t u, size_t col_stride, Fe<FP> beta, Fe<FP> gamma, U128* __restrict__ z) {
  using F = Fe<FP>;
  const size_t col = 2 * col_stride * blockIdx.y;
  const uint32_t lo = (blockIdx.x * 256 + threadIdx.x) * LOOKUP_RUN;
  if (lo > u) return;
  F num[LOOKUP_RUN], den[LOOKUP_RUN], pre[LOOKUP_RUN];
  bool zero[LOOKUP_RUN];
  F acc = F::one();
#pragma unroll
  for (int k = 0; k < LOOKUP_RUN; k++) {
    const uint32_t i = lo + k;
    num[k] = den[k] = F::one();
    if (i < u) {
      const size_t at = col + 2 * (size_t)i;
      num[k] = fe_mul(fe_add(fe_load<FP>(input + at), beta), fe_add(fe_load<FP>(table + at), gamma));
      den[k] = fe_mul(fe_add(fe_load<FP>(pin + at), beta), fe_add(fe_load<FP>(ptab + at), gamma));
    }
    zero[k] = den[k].is_zero();
    if (zero[k]) den[k] = F::one();
    pre[k] = acc;
    acc = fe_mul(acc, den[k]);
  }
  F inv = fe_inv(acc);
#pragma unroll
  for (int k = LOOKUP_RUN - 1; k >= 0; k--) {
    const uint32_t i = lo + k;
    if (i <= u) fe_store<FP>(z + col + 2 * (size_t)i, zero[k] ? F::zero() : fe_mul(num[k], fe_mul(pre[k], inv)));
    inv = fe_mul(inv, den[k]);
  }
}

template <class FP>
hipError_t lookup_ratio_launch(const void* d_input, const void* d_table, const void* d_pin, const void* d_ptab, size_t u,
                               size_t col_stride, size_t m, const uint64_t beta[4], const uint64_t gamma[4], void* d_z, hipStream_t s) {
  Fe<FP> b, g;
  memcpy(b.v, beta, 32);
  memcpy(g.v, gamma, 32);
  const size_t threads = (u + 1 + LOOKUP_RUN - 1) / LOOKUP_RUN;
  hipLaunchKernelGGL(lookup_ratio_kernel<FP>, dim3((unsigned)((threads + 255) / 256), (unsigned)m), dim3(256), 0, s, (const U128*)d_input,
                     (const U128*)d_table, (const U128*)d_pin, (const U128*)d_ptab, (uint32_t)u, col_stride, b, g, (U128*)d_z);
  return hipGetLastError();
}

}  // namespace h2
