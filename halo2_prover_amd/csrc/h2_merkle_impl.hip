// h2_merkle_impl.hip -- the kernels and launchers of a resident Poseidon Merkle tree (h2_poseidon_quad.hpp) and of the wide
// Poseidon family (h2_poseidon_wide.hpp: widths 5 and 9, 4-ary and 8-ary trees) for ONE curve's scalar field (selected by -DH2_CURVE_ID, as h2_curve_impl.hip).  A translation unit of its own: the code objects of
// h2_curve_impl.hip -- the MSM and NTT kernels of the registered path -- are what they were before these kernels existed.
#include "h2_poseidon_quad.hpp"
#include "h2_poseidon_wide.hpp"

#include <algorithm>
#include <cstring>      // before rocprim: its texture iterator calls memset without including this

#include <rocprim/rocprim.hpp>

#ifndef H2_CURVE_ID
#error "compile with -DH2_CURVE_ID=0 (bn254), 1 (pallas) or 2 (vesta)"
#endif

namespace h2 {
namespace {

#if H2_CURVE_ID == 0
using FS = typename BN254_CURVE::Scalar;
#elif H2_CURVE_ID == 1
using FS = typename PALLAS_CURVE::Scalar;
#else
using FS = typename VESTA_CURVE::Scalar;
#endif

Fe29<FS> poseidon_capacity(const uint64_t cap_mont[4]) {
  Fe<FS> c;
  memcpy(c.v, cap_mont, 32);
  return fe29_from_api(c);
}
unsigned merkle_grid(size_t items, bool quad) {
  const size_t per_block = quad ? POSEIDON_THREADS / 4 : POSEIDON_THREADS;
  return (unsigned)std::min<size_t>((items + per_block - 1) / per_block, POSEIDON_MAX_BLOCKS);
}
hipError_t poseidon_merkle_paths_launch(const void* d_leaves, const void* d_nodes, uint32_t depth, const void* d_indices, size_t n,
                                        void* d_paths, void* d_status, hipStream_t s) {
  hipLaunchKernelGGL(poseidon_merkle_paths_kernel, dim3(merkle_grid(n * depth, false)), dim3(POSEIDON_THREADS), 0, s, (const U128*)d_leaves,
                     (const U128*)d_nodes, depth, (const uint32_t*)d_indices, n, (U128*)d_paths, (uint32_t*)d_status);
  return hipGetLastError();
}
// quad_max: launches of fewer items than this run four lanes per hash, the others one (0: never, SIZE_MAX: always)
hipError_t poseidon_merkle_verify_launch(const void* d_leaf_values, const void* d_indices, const void* d_paths, uint32_t depth, size_t n,
                                         const void* d_root, void* d_roots_out, void* d_status, const uint64_t cap2_mont[4],
                                         const void* d_table, uint32_t r_f, uint32_t r_p, size_t quad_max, hipStream_t s) {
  const Fe29<FS> cap2 = poseidon_capacity(cap2_mont);
  if (n < quad_max)
    hipLaunchKernelGGL((poseidon_merkle_verify_kernel<FS, true>), dim3(merkle_grid(n, true)), dim3(POSEIDON_THREADS), 0, s,
                       (const U128*)d_leaf_values, (const uint32_t*)d_indices, (const U128*)d_paths, depth, n, (const U128*)d_root,
                       (U128*)d_roots_out, (uint32_t*)d_status, cap2, (const Fe29<FS>*)d_table, r_f, r_p);
  else
    hipLaunchKernelGGL((poseidon_merkle_verify_kernel<FS, false>), dim3(merkle_grid(n, false)), dim3(POSEIDON_THREADS), 0, s,
                       (const U128*)d_leaf_values, (const uint32_t*)d_indices, (const U128*)d_paths, depth, n, (const U128*)d_root,
                       (U128*)d_roots_out, (uint32_t*)d_status, cap2, (const Fe29<FS>*)d_table, r_f, r_p);
  return hipGetLastError();
}
// The update's scratch: keys and positions of the n items, unsorted and sorted, and what the sort asks for
struct MerkleUpdateScratch {
  size_t off_keys, off_pos, off_keys_sorted, off_pos_sorted, off_sort, sort_bytes, total;
};
hipError_t merkle_update_scratch(size_t n, uint32_t depth, MerkleUpdateScratch* out) {
  const size_t col = (4 * n + 255) & ~(size_t)255;
  MerkleUpdateScratch w{0, col, 2 * col, 3 * col, 4 * col, 0, 0};
  const hipError_t e = rocprim::radix_sort_pairs(nullptr, w.sort_bytes, (const uint32_t*)nullptr, (uint32_t*)nullptr,
                                                 (const uint32_t*)nullptr, (uint32_t*)nullptr, n, 0, depth + 1);
  w.total = w.off_sort + ((w.sort_bytes + 255) & ~(size_t)255);
  *out = w;
  return e;
}
size_t poseidon_merkle_update_scratch(size_t n, uint32_t depth) {
  MerkleUpdateScratch w;
  return merkle_update_scratch(n, depth, &w) == hipSuccess ? w.total : 0;
}
hipError_t poseidon_merkle_update_launch(void* d_leaves, void* d_nodes, uint32_t depth, const void* d_indices, const void* d_values,
                                         size_t n, void* d_status, const uint64_t cap2_mont[4], const void* d_table, uint32_t r_f,
                                         uint32_t r_p, size_t quad_max, void* d_scratch, size_t scratch_bytes, hipStream_t s) {
  MerkleUpdateScratch w;
  if (hipError_t e = merkle_update_scratch(n, depth, &w); e != hipSuccess) return e;
  if (depth == 0 || depth > 30 || n == 0 || n > ((size_t)1 << 31) || w.total > scratch_bytes) return hipErrorInvalidValue;
  const Fe29<FS> cap2 = poseidon_capacity(cap2_mont);
  const Fe29<FS>* table = (const Fe29<FS>*)d_table;
  uint32_t* keys = (uint32_t*)((char*)d_scratch + w.off_keys);
  uint32_t* pos = (uint32_t*)((char*)d_scratch + w.off_pos);
  uint32_t* keys_sorted = (uint32_t*)((char*)d_scratch + w.off_keys_sorted);
  uint32_t* pos_sorted = (uint32_t*)((char*)d_scratch + w.off_pos_sorted);
  U128* leaves = (U128*)d_leaves;
  U128* nodes = (U128*)d_nodes;
  hipLaunchKernelGGL(poseidon_merkle_update_keys_kernel<FS>, dim3(merkle_grid(n, false)), dim3(POSEIDON_THREADS), 0, s,
                     (const uint32_t*)d_indices, (const U128*)d_values, n, depth, keys, pos, (uint32_t*)d_status);
  // stable, on the bits a leaf index has and the one above them: MERKLE_NO_KEY ends up behind every index
  if (hipError_t e = rocprim::radix_sort_pairs((char*)d_scratch + w.off_sort, w.sort_bytes, (const uint32_t*)keys, keys_sorted,
                                               (const uint32_t*)pos, pos_sorted, n, 0, depth + 1, s);
      e != hipSuccess)
    return e;
  hipLaunchKernelGGL(poseidon_merkle_update_leaves_kernel, dim3(merkle_grid(n, false)), dim3(POSEIDON_THREADS), 0, s,
                     (const uint32_t*)keys_sorted, (const uint32_t*)pos_sorted, n, (const U128*)d_values, leaves, (uint32_t*)d_status);
  const bool quad_top = quad_max > 0;
  const uint32_t top = quad_top ? POSEIDON_TOP_QUAD : POSEIDON_TOP_LANE;
  uint32_t l = 0;
  for (; ((uint32_t)1 << (depth - 1 - l)) > top; l++) {
    const size_t width = (size_t)1 << (depth - 1 - l);
    const bool by_node = width <= n;
    const size_t items = by_node ? width : n;
    const U128* below = l == 0 ? leaves : nodes + 2 * merkle_level_offset(depth, l - 1);
    U128* level = nodes + 2 * merkle_level_offset(depth, l);
    if (items < quad_max)
      hipLaunchKernelGGL((poseidon_merkle_level_kernel<FS, true>), dim3(merkle_grid(items, true)), dim3(POSEIDON_THREADS), 0, s,
                         (const uint32_t*)keys_sorted, n, l, items, by_node, below, level, cap2, table, r_f, r_p);
    else
      hipLaunchKernelGGL((poseidon_merkle_level_kernel<FS, false>), dim3(merkle_grid(items, false)), dim3(POSEIDON_THREADS), 0, s,
                         (const uint32_t*)keys_sorted, n, l, items, by_node, below, level, cap2, table, r_f, r_p);
  }
  if (quad_top)
    hipLaunchKernelGGL((poseidon_merkle_top_kernel<FS, true>), dim3(1), dim3(POSEIDON_THREADS), 0, s, (const uint32_t*)keys_sorted, n,
                       depth, l, (const U128*)leaves, nodes, cap2, table, r_f, r_p);
  else
    hipLaunchKernelGGL((poseidon_merkle_top_kernel<FS, false>), dim3(1), dim3(POSEIDON_THREADS), 0, s, (const uint32_t*)keys_sorted, n,
                       depth, l, (const U128*)leaves, nodes, cap2, table, r_f, r_p);
  return hipGetLastError();
}

const MerkleOps OPS = {poseidon_merkle_paths_launch, poseidon_merkle_verify_launch, poseidon_merkle_update_scratch,
                       poseidon_merkle_update_launch};

// ---- the wide family (h2_poseidon_wide.hpp) ------------------------------------------------------------------------------
template <int T>
void wide_hash_enqueue(const U128* d_msgs, uint32_t len, size_t msg_stride, size_t n, U128* d_out, const Fe29<FS>& cap,
                       const void* d_table, uint32_t r_f, uint32_t r_p, size_t chain_min_n, hipStream_t s) {
  if constexpr (chain29::covers<FS>()) {
    if (n >= chain_min_n) {
      hipLaunchKernelGGL((poseidon_wide_hash_kernel<FS, T, Fe29Chain>), dim3(merkle_grid(n, false)), dim3(POSEIDON_THREADS), 0, s, d_msgs,
                         len, msg_stride, n, d_out, cap, (const Fe29<FS>*)d_table, r_f, r_p);
      return;
    }
  }
  hipLaunchKernelGGL((poseidon_wide_hash_kernel<FS, T, Fe29Compiler>), dim3(merkle_grid(n, false)), dim3(POSEIDON_THREADS), 0, s, d_msgs,
                     len, msg_stride, n, d_out, cap, (const Fe29<FS>*)d_table, r_f, r_p);
}
template <int T>
hipError_t wide_merkle_enqueue(const void* d_leaves, uint32_t depth, void* d_nodes, const Fe29<FS>& cap, const void* d_table,
                               uint32_t r_f, uint32_t r_p, uint32_t tail, size_t chain_min_n, hipStream_t s) {
  constexpr uint32_t ARITY = T - 1, LG = ARITY == 8 ? 3 : 2;
  if (depth == 0 || LG * depth > 30 || tail == 0 || tail > POSEIDON_MERKLE_TAIL_MAX) return hipErrorInvalidValue;
  const U128* in = (const U128*)d_leaves;
  U128* out = (U128*)d_nodes;
  size_t w = merkle_wide_pow(LG, depth - 1);       // nodes of the level being written
  for (; w > tail; w /= ARITY) {                   // one launch per level; what is left is a power of the arity <= tail
    wide_hash_enqueue<T>(in, ARITY, ARITY, w, out, cap, d_table, r_f, r_p, chain_min_n, s);
    in = out;
    out += 2 * w;
  }
  hipLaunchKernelGGL((poseidon_wide_merkle_tail_kernel<FS, T>), dim3(1), dim3(POSEIDON_THREADS), 0, s, in, out, (uint32_t)w, cap,
                     (const Fe29<FS>*)d_table, r_f, r_p);
  return hipGetLastError();
}
template <int T>
hipError_t wide_verify_enqueue(const void* d_leaf_values, const void* d_indices, const void* d_paths, uint32_t depth, size_t n,
                               const void* d_root, void* d_roots_out, void* d_status, const Fe29<FS>& cap, const void* d_table,
                               uint32_t r_f, uint32_t r_p, hipStream_t s) {
  hipLaunchKernelGGL((poseidon_wide_merkle_verify_kernel<FS, T>), dim3(merkle_grid(n, false)), dim3(POSEIDON_THREADS), 0, s,
                     (const U128*)d_leaf_values, (const uint32_t*)d_indices, (const U128*)d_paths, depth, n, (const U128*)d_root,
                     (U128*)d_roots_out, (uint32_t*)d_status, cap, (const Fe29<FS>*)d_table, r_f, r_p);
  return hipGetLastError();
}
template <int T>
hipError_t wide_permute_enqueue(int form, const void* d_in, void* d_out, size_t n, const void* d_table, uint32_t r_f, uint32_t r_p,
                                hipStream_t s) {
  if (form == 0 ? POSEIDON_WIDE_SPARSE<T> : form == 2)
    hipLaunchKernelGGL((poseidon_wide_permute_kernel<FS, T, true>), dim3(merkle_grid(n, false)), dim3(POSEIDON_THREADS), 0, s,
                       (const U128*)d_in, (U128*)d_out, n, (const Fe29<FS>*)d_table, r_f, r_p);
  else
    hipLaunchKernelGGL((poseidon_wide_permute_kernel<FS, T, false>), dim3(merkle_grid(n, false)), dim3(POSEIDON_THREADS), 0, s,
                       (const U128*)d_in, (U128*)d_out, n, (const Fe29<FS>*)d_table, r_f, r_p);
  return hipGetLastError();
}
hipError_t wide_permute_launch(uint32_t width, int form, const void* d_in, void* d_out, size_t n, const void* d_table, uint32_t r_f,
                               uint32_t r_p, hipStream_t s) {
  if (form < 0 || form > 2) return hipErrorInvalidValue;
  if (width == 5) return wide_permute_enqueue<5>(form, d_in, d_out, n, d_table, r_f, r_p, s);
  if (width == 9) return wide_permute_enqueue<9>(form, d_in, d_out, n, d_table, r_f, r_p, s);
  return hipErrorInvalidValue;
}
hipError_t wide_hash_launch(uint32_t width, const void* d_msgs, uint32_t len, size_t msg_stride, size_t n, void* d_out,
                            const uint64_t cap_mont[4], const void* d_table, uint32_t r_f, uint32_t r_p, size_t chain_min_n,
                            hipStream_t s) {
  const Fe29<FS> cap = poseidon_capacity(cap_mont);
  if (width == 5) wide_hash_enqueue<5>((const U128*)d_msgs, len, msg_stride, n, (U128*)d_out, cap, d_table, r_f, r_p, chain_min_n, s);
  else if (width == 9) wide_hash_enqueue<9>((const U128*)d_msgs, len, msg_stride, n, (U128*)d_out, cap, d_table, r_f, r_p, chain_min_n, s);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}
hipError_t wide_merkle_launch(uint32_t width, const void* d_leaves, uint32_t depth, void* d_nodes, const uint64_t cap_mont[4],
                              const void* d_table, uint32_t r_f, uint32_t r_p, uint32_t tail, size_t chain_min_n, hipStream_t s) {
  const Fe29<FS> cap = poseidon_capacity(cap_mont);
  if (width == 5) return wide_merkle_enqueue<5>(d_leaves, depth, d_nodes, cap, d_table, r_f, r_p, tail, chain_min_n, s);
  if (width == 9) return wide_merkle_enqueue<9>(d_leaves, depth, d_nodes, cap, d_table, r_f, r_p, tail, chain_min_n, s);
  return hipErrorInvalidValue;
}
hipError_t wide_paths_launch(uint32_t width, const void* d_leaves, const void* d_nodes, uint32_t depth, const void* d_indices, size_t n,
                             void* d_paths, void* d_status, hipStream_t s) {
  const uint32_t lg = width == 9 ? 3 : width == 5 ? 2 : 0;
  if (lg == 0 || depth == 0 || lg * depth > 30) return hipErrorInvalidValue;
  hipLaunchKernelGGL(poseidon_wide_merkle_paths_kernel, dim3(merkle_grid(n * depth * (width - 2), false)), dim3(POSEIDON_THREADS), 0, s,
                     (const U128*)d_leaves, (const U128*)d_nodes, lg, depth, (const uint32_t*)d_indices, n, (U128*)d_paths,
                     (uint32_t*)d_status);
  return hipGetLastError();
}
hipError_t wide_verify_launch(uint32_t width, const void* d_leaf_values, const void* d_indices, const void* d_paths, uint32_t depth,
                              size_t n, const void* d_root, void* d_roots_out, void* d_status, const uint64_t cap_mont[4],
                              const void* d_table, uint32_t r_f, uint32_t r_p, hipStream_t s) {
  const Fe29<FS> cap = poseidon_capacity(cap_mont);
  if (depth == 0 || (width == 9 ? 3 : 2) * depth > 30) return hipErrorInvalidValue;
  if (width == 5) return wide_verify_enqueue<5>(d_leaf_values, d_indices, d_paths, depth, n, d_root, d_roots_out, d_status, cap, d_table, r_f, r_p, s);
  if (width == 9) return wide_verify_enqueue<9>(d_leaf_values, d_indices, d_paths, depth, n, d_root, d_roots_out, d_status, cap, d_table, r_f, r_p, s);
  return hipErrorInvalidValue;
}
// host: poseidon_wide_permute / poseidon_wide_hash on a host copy of the table
template <int T, bool SPARSE>
int wide_selftest_t(int op, uint32_t len, uint32_t r_f, uint32_t r_p, const int32_t* table, const uint64_t* cap_mont, const uint64_t* in,
                    uint64_t* out) {
  const Fe29<FS>* tb = (const Fe29<FS>*)table;
  if (op == 0) {
    Fe29<FS> st[T];
    for (int j = 0; j < T; j++) {
      Fe<FS> a;
      memcpy(a.v, in + 4 * j, 32);
      st[j] = fe29_from_api(a);
    }
    poseidon_wide_permute<FS, T, Fe29Compiler, SPARSE>(st, tb, r_f, r_p);
    for (int j = 0; j < T; j++) {
      const Fe<FS> r = fe29_to_api(st[j]);
      memcpy(out + 4 * j, r.v, 32);
    }
    return 0;
  }
  if (op == 1 && len >= 1 && SPARSE == POSEIDON_WIDE_SPARSE<T>) {
    const Fe<FS> r = fe29_to_api(poseidon_wide_hash<FS, T>((const U128*)in, len, poseidon_capacity(cap_mont), tb, r_f, r_p));
    memcpy(out, r.v, 32);
    return 0;
  }
  return -1;
}
int wide_selftest(uint32_t width, int form, int op, uint32_t len, uint32_t r_f, uint32_t r_p, const int32_t* table,
                  const uint64_t* cap_mont, const uint64_t* in, uint64_t* out) {
  if (form < 0 || form > 2) return -1;
  const bool sparse = form == 0 ? (width == 5 ? POSEIDON_WIDE_SPARSE<5> : POSEIDON_WIDE_SPARSE<9>) : form == 2;
  if (width == 5)
    return sparse ? wide_selftest_t<5, true>(op, len, r_f, r_p, table, cap_mont, in, out)
                  : wide_selftest_t<5, false>(op, len, r_f, r_p, table, cap_mont, in, out);
  if (width == 9)
    return sparse ? wide_selftest_t<9, true>(op, len, r_f, r_p, table, cap_mont, in, out)
                  : wide_selftest_t<9, false>(op, len, r_f, r_p, table, cap_mont, in, out);
  return -1;
}

const PoseidonWideOps WIDE_OPS = {wide_permute_launch, wide_hash_launch, wide_merkle_launch, wide_paths_launch, wide_verify_launch,
                                  wide_selftest};

}  // namespace

#if H2_CURVE_ID == 0
const PoseidonWideOps* poseidon_wide_ops_bn254() { return &WIDE_OPS; }
#elif H2_CURVE_ID == 1
const PoseidonWideOps* poseidon_wide_ops_pallas() { return &WIDE_OPS; }
#else
const PoseidonWideOps* poseidon_wide_ops_vesta() { return &WIDE_OPS; }
#endif
#if H2_CURVE_ID == 0
const MerkleOps* merkle_ops_bn254() { return &OPS; }
#elif H2_CURVE_ID == 1
const MerkleOps* merkle_ops_pallas() { return &OPS; }
#else
const MerkleOps* merkle_ops_vesta() { return &OPS; }
#endif

}  // namespace h2
