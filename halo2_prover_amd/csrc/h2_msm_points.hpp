// h2_msm_points.hpp -- table-free Pippenger MSM over points the caller passes WITH the call (h2_msm_points*).
//
// best_multiexp(coeffs, bases) takes whatever slice it is given; the resident-table MSM of h2_msm.hpp wants its bases
// registered first, which builds T[w][i] = 2^(off_w) P_i for every window -- ~1 ms at 2^16 against 0.4 ms for the MSM
// itself.  For bases used once there is no table here: every window keeps its OWN bucket set and the window results are
// combined by doublings at the end, as in the textbook algorithm.
//
// The sort and the whole tail of h2_msm.hpp do not care what a "column" is: window w of scalar column `col` is simply
// VIRTUAL COLUMN col * W + w of a one-window MSM with B = 2^(c-1) buckets.  So only three things are new:
//  * pack: the n points in the API form -> the form a table entry has (window 0 of a table: T[0][i] = P_i, 64 bytes);
//    the accumulate kernel gathers from it unchanged, a sorted entry is i | sign;
//  * the sort front: a block loads and decomposes each scalar of its tile ONCE (MsmDigits) and files the digit of window w
//    under key (col * W + w) * B + |d| - 1 -- the tile's histogram is W * B words of LDS, which bounds the window width
//    (msm_points_geometry).  gcounts, tile_base and the sorted entries leave in the layout msm_digits_kernel /
//    msm_scatter_kernel use for m * W columns, so scan, keys pass, accumulate, fix-up, weights and final are the kernels of
//    h2_msm.hpp on m * W columns (msm_launch_scan, msm_launch_back);
//  * combine: one quad per scalar column folds its W window results from the top window down,
//    acc = 2^(width_w) acc + R_w, and writes the Jacobian result in the API form.
//
// The points are NOT checked to be on the curve (best_multiexp does not check either).  Every index these kernels form
// depends on the scalars and on n only -- a digit's bucket, a scalar's index -- so a bad point gives a wrong sum and
// never an out-of-range access.
#pragma once
#include "h2_msm.hpp"

namespace h2 {

// the front's LDS histogram, W * B words: what the one-level sort may use per CU (MSM_MAX_C_ONE_LEVEL: 128 KiB)
constexpr size_t MSM_POINTS_LDS_CAP = (size_t)4 << (MSM_MAX_C_ONE_LEVEL - 1);
constexpr uint32_t MSM_POINTS_MAX_C = 11;      // 24 windows x 1024 buckets x 4 bytes = 96 KiB; 12 bits would need 176 KiB
constexpr uint32_t MSM_POINTS_MIN_C = 6;       // the tail's smallest bucket set, as in msm_geometry (tuning builds; the rule gives >= 8)
// the largest n one call takes: a column's W * n sorted entries are indexed with 31 bits, and from 2^20 terms on the
// rule below gives W = 24 windows (24 * 2^26 < 2^31)
constexpr size_t MSM_POINTS_MAX_N = (size_t)1 << 26;

// Window width of the table-free MSM.  Not msm_geometry's: there all windows share one bucket set, here every window
// pays for its own B buckets in the tail (~16 point operations per bucket, W times over), so the optimum is narrower.
// Rule: c = log2 n - 9, between 8 and 11 bits: 8 bits up to 2^17 terms, 9 / 10 at 2^18 / 2^19, 11 from 2^20.
// Swept on the GPU at 2^10, 2^13, 2^16 and 2^20 with 1 and 4 columns (profiles/msm_points_window_sweep.txt,
// tools/msm_points_bench.py --sweep on a tuning build; best of seven, ms): at 2^10 c = 6 .. 9 are within 0.03 of each
// other (0.82 at 8); at 2^13 8 bits are best (0.85 against 0.88 / 0.89 / 0.91 at 7 / 9 / 10); at 2^16 8 bits again for one
// column (1.02 against 1.06 / 1.07 / 1.18 at 9 / 10 / 11) and 8 .. 10 level for four (1.51 / 1.51 / 1.48); at 2^20 every
// bit still pays, 3.73 / 3.75 / 3.44 / 3.18 at 8 / 9 / 10 / 11 (four columns 11.6 / 11.3 / 10.3 / 9.7).  Below 2^16 the call
// is the combine's ~255 dependent doublings (~0.7 of 0.85 ms) whatever the width.  11 bits is the ceiling whatever n is:
// W * B words of histogram must fit MSM_POINTS_LDS_CAP, and at 12 bits (22 x 2048 words) they do not -- the sizes
// between 2^16 and 2^20 are interpolated, and running the windows in groups for wider ones is not built.
inline MsmGeom msm_points_geometry(size_t n, uint32_t nbits) {
  uint32_t lg = 0;
  while (((size_t)1 << (lg + 1)) <= n) lg++;
  int c = std::max(8, (int)lg - 9);
  c = tune_int("H2_TUNE_POINTS_C", c);      // tuning builds only (h2_tune.hpp)
  if (c < (int)MSM_POINTS_MIN_C) c = (int)MSM_POINTS_MIN_C;
  if (c > (int)MSM_POINTS_MAX_C) c = (int)MSM_POINTS_MAX_C;
  MsmGeom g{};
  g.nbits = nbits;
  const uint32_t total = nbits + 1;  // one spare bit: the top window never carries out
  g.W = (total + c - 1) / c;
  const uint32_t base = total / g.W, extra = total % g.W;
  g.wbase = base;
  g.wextra = extra;
  uint32_t o = 0;
  for (uint32_t w = 0; w < g.W; w++) {
    g.off[w] = (uint8_t)o;
    g.width[w] = (uint8_t)(base + (w < extra ? 1 : 0));
    o += g.width[w];
  }
  g.c = base + (extra ? 1 : 0);
  g.B = 1u << (g.c - 1);
  return g;
}
// a virtual column's geometry: one window, the same bucket count
inline MsmGeom msm_points_virtual(const MsmGeom& g) {
  MsmGeom v{};
  v.c = g.c;
  v.W = 1;
  v.B = g.B;
  v.nbits = g.nbits;
  v.wbase = g.c;
  v.wextra = 0;
  v.off[0] = 0;
  v.width[0] = (uint8_t)g.c;
  return v;
}
inline MsmWorkspace msm_points_workspace(size_t n, size_t m, const MsmGeom& g, uint32_t guard = 0) {
  const MsmPointsShape shape{m, g.W};
  return msm_workspace(n, m * g.W, msm_points_virtual(g), guard, n, true, &shape);
}
// scalar columns one launch sequence takes (0: one column is already too long); a wider call runs in groups of that many
inline size_t msm_points_cols_per_launch(const MsmGeom& g, size_t n) {
  const uint64_t by_entries = ((1ull << 31) - 1) / ((uint64_t)g.W * n);
  const uint64_t by_keys = std::min<uint64_t>(((1ull << 31) - 1) / ((uint64_t)g.W * g.B), 65535u / g.W);   // grid.y of the tail
  return (size_t)std::min(by_entries, by_keys);
}

// ---- pack: API-form points -> table entries ------------------------------------------------------------------------
template <class CV>
__global__ void __launch_bounds__(256)
msm_points_pack_kernel(const U128* __restrict__ points, U128* __restrict__ packed, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  affine29_store_table<CV>(packed + 4 * (size_t)i, affine_load<CV>(points + 4 * (size_t)i));
}

// ---- the sort front ------------------------------------------------------------------------------------------------
// Both kernels tile the m REAL columns (msm_tile_id over (tiles, m): XCD-grouped, surplus blocks dead) and file window
// w's digit under virtual column col * W + w.  LDS: W * B words; idx = w * B + bucket, so col * W * B + idx is the key.
// grid = msm_tile_grid(tiles, m).
template <class CV>
__global__ void __launch_bounds__(1024)
msm_points_digits_kernel(const U128* __restrict__ scalars, uint32_t* __restrict__ gcounts, uint32_t* __restrict__ tile_base,
                         uint32_t n, size_t col_stride /* elements */, uint32_t tile, uint32_t tiles, uint32_t m, MsmGeom g) {
  using S = typename CV::Scalar;
  extern __shared__ uint32_t hist[];
  const MsmTileId id = msm_tile_id(tiles, m);
  if (!id.live) return;
  const uint32_t WB = g.W * g.B, log_b = g.c - 1;
  for (uint32_t b = threadIdx.x; b < WB; b += blockDim.x) hist[b] = 0;
  __syncthreads();
  const uint32_t lo = id.tile * tile, hi = min(lo + tile, n);
  for (uint32_t i = lo + threadIdx.x; i < hi; i += blockDim.x) {
    MsmDigits dg(fe_from_mont(fe_load<S>(scalars + 2 * (col_stride * id.col + i))).v);
    for (uint32_t w = 0; w < g.W; w++) {
      const uint32_t enc = dg.next(g, w);
      if (enc) atomicAdd(&hist[(w << log_b) + (enc & ~MSM_SIGN) - 1], 1u);
    }
  }
  __syncthreads();
  const size_t K = (size_t)m * WB;
  uint32_t* gc = gcounts + (size_t)id.group * K + (size_t)id.col * WB;
  for (uint32_t idx = threadIdx.x; idx < WB; idx += blockDim.x) {
    const uint32_t h = hist[idx], w = idx >> log_b, b = idx & (g.B - 1);
    const size_t vcol = (size_t)id.col * g.W + w;
    tile_base[(vcol * tiles + id.tile) * g.B + b] = h ? atomicAdd(&gc[idx], h) : 0u;
  }
}

// sorted_ref[pos] = i | sign: the entry indexes the packed points
template <class CV>
__global__ void __launch_bounds__(1024)
msm_points_scatter_kernel(const U128* __restrict__ scalars, const uint32_t* __restrict__ offsets,
                          const uint32_t* __restrict__ gcounts, const uint32_t* __restrict__ tile_base,
                          uint32_t* __restrict__ sorted_ref, uint32_t n, size_t col_stride /* elements */, uint32_t tile,
                          uint32_t tiles, uint32_t m, MsmGeom g) {
  using S = typename CV::Scalar;
  extern __shared__ uint32_t hist[];
  const MsmTileId id = msm_tile_id(tiles, m);
  if (!id.live) return;
  const uint32_t WB = g.W * g.B, log_b = g.c - 1;
  const size_t K = (size_t)m * WB;
  const uint32_t* gc = gcounts + (size_t)id.col * WB;
  const uint32_t* of = offsets + (size_t)id.col * WB;
  for (uint32_t idx = threadIdx.x; idx < WB; idx += blockDim.x) {
    const uint32_t w = idx >> log_b, b = idx & (g.B - 1);
    const size_t vcol = (size_t)id.col * g.W + w;
    uint32_t at = of[idx] + tile_base[(vcol * tiles + id.tile) * g.B + b];
    for (uint32_t x = 0; x < id.group; x++) at += gc[x * K + idx];       // the groups below this one come first in the list
    hist[idx] = at;
  }
  __syncthreads();
  const uint32_t lo = id.tile * tile, hi = min(lo + tile, n);
  for (uint32_t i = lo + threadIdx.x; i < hi; i += blockDim.x) {
    MsmDigits dg(fe_from_mont(fe_load<S>(scalars + 2 * (col_stride * id.col + i))).v);
    for (uint32_t w = 0; w < g.W; w++) {
      const uint32_t enc = dg.next(g, w);
      if (enc) {
        const uint32_t pos = atomicAdd(&hist[(w << log_b) + (enc & ~MSM_SIGN) - 1], 1u);
        sorted_ref[pos] = i | (enc & MSM_SIGN);
      }
    }
  }
}

// ---- combine: out[col] = sum_w 2^(off_w) R[col * W + w] --------------------------------------------------------------
// One quad per scalar column (h2_curve_quad.hpp), from the top window down: about nbits doublings and W additions, the
// columns side by side.  Identity window results pass through the group law as they are, and an identity total leaves as
// z = 0.  All lanes of a quad stay active: the quads past the last column fold identities.
template <class CV>
__global__ void __launch_bounds__(64)
msm_points_combine_kernel(const uint32_t* __restrict__ results /* m * W points, XYZZ on the working form */,
                          U128* __restrict__ out_jac, uint32_t m, MsmGeom g) {
  __builtin_amdgcn_s_setprio(3);   // a dependent chain on a mostly idle SIMD
  using P = Xyzz29<CV>;
  using F = Fe29<typename CV::Base>;
  using B = typename CV::Base;
  const uint32_t col = blockIdx.x * 16 + (threadIdx.x >> 2), q = threadIdx.x & 3u;
  const bool live = col < m;
  P acc = P::identity();
#pragma nounroll
  for (uint32_t w = g.W; w-- > 0;) {
    const uint32_t width = g.wbase + (w < g.wextra ? 1u : 0u);
#pragma nounroll
    for (uint32_t k = 0; k < width; k++) acc = xyzz29_double_quad(acc);
    const P r = live ? xyzz29_load<CV>(results + XYZZ29_WORDS * ((size_t)col * g.W + w)) : P::identity();
    acc = xyzz29_add_quad(acc, r);
  }
  // X zz, Y zzz, zz on lanes 0, 1, 2 of the quad, each lane converting and storing its own coordinate
  const F one = fe29_one<CV>();
  const F prod = fe29_mul(quad_select(q, acc.x, acc.y, acc.zz, acc.zz), quad_select(q, acc.zz, acc.zzz, one, one));
  Fe<B> v = fe29_to_api(prod);
  if (acc.is_identity()) v = Fe<B>::zero();
  if (live && q < 3) fe_store<B>(out_jac + 6 * (size_t)col + 2 * q, v);
}

// ---- launch proof ----------------------------------------------------------------------------------------------------
// msm_check on the m * W virtual columns covers everything behind the sort front (and tile_base, gcounts and the scan for
// that many columns); the conditions of the front itself and of the combine come on top.  Null, or the first violated
// condition: nothing is enqueued then.
#define MSM_REQUIRE(cond) \
  do {                    \
    if (!(cond)) return #cond; \
  } while (0)
inline const char* msm_points_check(const MsmWorkspace& ws, const MsmGeom& g, size_t n, size_t m, size_t col_stride,
                                    size_t arena_bytes) {
  MSM_REQUIRE(n >= 1 && m >= 1 && n <= MSM_POINTS_MAX_N);
  MSM_REQUIRE(col_stride >= n);
  MSM_REQUIRE(g.c >= MSM_POINTS_MIN_C && g.c <= MSM_POINTS_MAX_C && g.W >= 1 && g.W <= MSM_MAX_WINDOWS);
  MSM_REQUIRE(g.B == (1u << (g.c - 1)) && g.wbase >= 1 && g.wbase + (g.wextra ? 1u : 0u) == g.c && g.wextra < g.W);
  MSM_REQUIRE(g.wbase * g.W + g.wextra == g.nbits + 1);                  // the windows cover the scalar and the spare bit
  MSM_REQUIRE((uint64_t)m * g.W <= 65535);
  const MsmGeom v = msm_points_virtual(g);
  if (const char* broken = msm_check(ws, v, n, m * g.W, col_stride, (uint32_t)n, arena_bytes)) return broken;
  MSM_REQUIRE(!ws.sort2 && !ws.staged);                                  // the front is the direct one-level sort
  MSM_REQUIRE((size_t)g.W * g.B * 4 <= MSM_POINTS_LDS_CAP);              // the tile's histogram: W * B words of LDS
  MSM_REQUIRE(n < (1ull << 31));                                         // an entry is i below the sign bit
  MSM_REQUIRE(ws.K == m * (size_t)g.W * g.B && ws.E == m * (size_t)g.W * n);
  const size_t tiles = (n + ws.tile - 1) / ws.tile;
  MSM_REQUIRE(ws.tile >= 1 && tiles * ws.tile >= n && tiles * m < (1ull << 31) - MSM_XCDS);
  MSM_REQUIRE(msm_tile_grid((uint32_t)tiles, (uint32_t)m) >= tiles * m);
  MSM_REQUIRE((m - 1) * col_stride + n <= (1ull << 40));                 // scalar index col_stride * col + i
  auto bytes_at = [&](size_t off) -> size_t {
    for (uint32_t r = 0; r < ws.n_regions; r++)
      if (off >= ws.regions[r].off && off < ws.regions[r].off + ws.regions[r].bytes)
        return ws.regions[r].off + ws.regions[r].bytes - off;
    return 0;
  };
  MSM_REQUIRE(bytes_at(ws.off_points) >= n * 64 && ws.off_points % 16 == 0);   // packed points: entry i at 64 i
  MSM_REQUIRE(bytes_at(ws.off_tile_base) >= tiles * m * g.W * g.B * 4);  // ((col W + w) tiles + tile) B + b
  MSM_REQUIRE(ws.off_gcounts + MSM_XCDS * m * (size_t)g.W * g.B * 4 <= ws.off_misc + ws.zero_bytes);
  MSM_REQUIRE(bytes_at(ws.off_tree2) >= m * g.W * (XYZZ29_WORDS * 4));   // the combine reads m * W results
  MSM_REQUIRE((n + 255) / 256 < (1ull << 31) && (m + 15) / 16 < (1ull << 31));
  return nullptr;
}
#undef MSM_REQUIRE

template <class CV>
inline hipError_t msm_points_kernel_setup() {
  hipError_t e;
  if ((e = hipFuncSetAttribute((const void*)msm_points_digits_kernel<CV>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)MSM_POINTS_LDS_CAP)) != hipSuccess) return e;
  return hipFuncSetAttribute((const void*)msm_points_scatter_kernel<CV>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)MSM_POINTS_LDS_CAP);
}

// Enqueue m table-free MSMs of n terms: out_j = sum_i scalars_j[i] points[i].  g = msm_points_geometry, ws =
// msm_points_workspace of (n, m, g), checked by msm_points_check.  m Jacobian points at d_out_jac.
template <class CV>
inline hipError_t msm_points_launch(const U128* d_points, const U128* d_scalars, size_t n, size_t col_stride, size_t m,
                                    const MsmGeom& g, char* ws_base, const MsmWorkspace& ws, hipStream_t stream, U128* d_out_jac,
                                    bool zeroed) {
  uint32_t* gcounts = (uint32_t*)(ws_base + ws.off_gcounts);
  uint32_t* offsets = (uint32_t*)(ws_base + ws.off_offsets);
  uint32_t* tile_base = (uint32_t*)(ws_base + ws.off_tile_base);
  uint32_t* sref = (uint32_t*)(ws_base + ws.off_ref);
  U128* packed = (U128*)(ws_base + ws.off_points);
  hipError_t e;
  if (!zeroed && (e = hipMemsetAsync(ws_base + ws.off_misc, 0, ws.zero_bytes, stream)) != hipSuccess) return e;
  hipLaunchKernelGGL(msm_points_pack_kernel<CV>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, d_points, packed, (uint32_t)n);
  const size_t lds = (size_t)g.W * g.B * 4;
  const uint32_t tiles = (uint32_t)((n + ws.tile - 1) / ws.tile);
  const uint32_t sort_grid = msm_tile_grid(tiles, (uint32_t)m);
  hipLaunchKernelGGL(msm_points_digits_kernel<CV>, dim3(sort_grid), dim3(MSM_SORT_THREADS), lds, stream, d_scalars, gcounts,
                     tile_base, (uint32_t)n, col_stride, ws.tile, tiles, (uint32_t)m, g);
  msm_launch_scan(ws_base, ws, stream);
  hipLaunchKernelGGL(msm_points_scatter_kernel<CV>, dim3(sort_grid), dim3(MSM_SORT_THREADS), lds, stream, d_scalars,
                     (const uint32_t*)offsets, (const uint32_t*)gcounts, (const uint32_t*)tile_base, sref, (uint32_t)n, col_stride,
                     ws.tile, tiles, (uint32_t)m, g);
  const MsmGeom v = msm_points_virtual(g);
  if ((e = msm_launch_back<CV>(packed, nullptr, 0, m * g.W, v, ws_base, ws, msm_keys_args(ws_base, ws), false, stream, nullptr,
                               nullptr, nullptr, nullptr)) != hipSuccess)
    return e;
  hipLaunchKernelGGL(msm_points_combine_kernel<CV>, dim3((unsigned)((m + 15) / 16)), dim3(64), 0, stream,
                     (const uint32_t*)(ws_base + ws.off_tree2), d_out_jac, (uint32_t)m, g);
  return hipGetLastError();
}

}  // namespace h2
