// h2_poseidon_impl.hip -- the kernels and launchers of the Poseidon family (h2_poseidon.hpp, h2_poseidon_merkle.hpp: widths
// 3, 5 and 9, the trees on them and the update of a resident binary tree) for ONE curve's scalar field (selected by
// -DH2_CURVE_ID, as h2_curve_impl.hip).  A translation unit of its own: the code objects of h2_curve_impl.hip -- the MSM and
// NTT kernels of the registered path -- hold no Poseidon kernel.
#include "h2_poseidon_merkle.hpp"

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

// n constants in the API form -> the kernels' table entries (working form, 9 limbs each); host
void poseidon_table(const uint64_t* api, size_t n, int32_t* out) {
  for (size_t i = 0; i < n; i++) {
    Fe<FS> a;
    memcpy(a.v, api + 4 * i, 32);
    const Fe29<FS> w = fe29_from_api(a);
    memcpy(out + 9 * i, w.v, 36);
  }
}
Fe29<FS> poseidon_capacity(const uint64_t cap_mont[4]) {
  Fe<FS> c;
  memcpy(c.v, cap_mont, 32);
  return fe29_from_api(c);
}
// blocks for `items` hashes of `lanes` lanes each (4: the quad form)
unsigned poseidon_grid(size_t items, uint32_t lanes = 1) {
  const size_t per_block = POSEIDON_THREADS / lanes;
  return (unsigned)std::min<size_t>((items + per_block - 1) / per_block, POSEIDON_MAX_BLOCKS);
}
// f(the width as a compile-time constant); a width that is not instantiated is hipErrorInvalidValue
template <class F>
hipError_t by_width(uint32_t width, F&& f) {
  if (width == 3) return f(std::integral_constant<int, 3>());
  if (width == 5) return f(std::integral_constant<int, 5>());
  if (width == 9) return f(std::integral_constant<int, 9>());
  return hipErrorInvalidValue;
}
// the partial rounds of a permutation launch or selftest: the sparse form? (width 3 has the dense one only)
template <int T>
bool poseidon_sparse(int form) { return T != 3 && (form == 0 ? POSEIDON_SPARSE<T> : form == 2); }

hipError_t poseidon_permute_launch(uint32_t width, int form, const void* d_in, void* d_out, size_t n, const void* d_table, uint32_t r_f,
                                   uint32_t r_p, hipStream_t s) {
  if (form < 0 || form > 2) return hipErrorInvalidValue;
  return by_width(width, [&](auto t) {
    constexpr int T = decltype(t)::value;
    if constexpr (T != 3) {
      if (poseidon_sparse<T>(form)) {
        hipLaunchKernelGGL((poseidon_permute_kernel<FS, T, true>), dim3(poseidon_grid(n)), dim3(POSEIDON_THREADS), 0, s, (const U128*)d_in,
                           (U128*)d_out, n, (const Fe29<FS>*)d_table, r_f, r_p);
        return hipGetLastError();
      }
    }
    hipLaunchKernelGGL((poseidon_permute_kernel<FS, T, false>), dim3(poseidon_grid(n)), dim3(POSEIDON_THREADS), 0, s, (const U128*)d_in,
                       (U128*)d_out, n, (const Fe29<FS>*)d_table, r_f, r_p);
    return hipGetLastError();
  });
}
template <int T>
void poseidon_hash_enqueue(const U128* d_msgs, uint32_t len, size_t msg_stride, size_t n, U128* d_out, const Fe29<FS>& cap,
                           const void* d_table, uint32_t r_f, uint32_t r_p, size_t chain_min_n, hipStream_t s) {
  if constexpr (chain29::covers<FS>()) {
    if (n >= chain_min_n) {
      hipLaunchKernelGGL((poseidon_hash_kernel<FS, T, Fe29Chain>), dim3(poseidon_grid(n)), dim3(POSEIDON_THREADS), 0, s, d_msgs, len,
                         msg_stride, n, d_out, cap, (const Fe29<FS>*)d_table, r_f, r_p);
      return;
    }
  }
  hipLaunchKernelGGL((poseidon_hash_kernel<FS, T, Fe29Compiler>), dim3(poseidon_grid(n)), dim3(POSEIDON_THREADS), 0, s, d_msgs, len,
                     msg_stride, n, d_out, cap, (const Fe29<FS>*)d_table, r_f, r_p);
}
hipError_t poseidon_hash_launch(uint32_t width, const void* d_msgs, uint32_t len, size_t msg_stride, size_t n, void* d_out,
                                const uint64_t cap_mont[4], const void* d_table, uint32_t r_f, uint32_t r_p, size_t chain_min_n,
                                hipStream_t s) {
  return by_width(width, [&](auto t) {
    poseidon_hash_enqueue<decltype(t)::value>((const U128*)d_msgs, len, msg_stride, n, (U128*)d_out, poseidon_capacity(cap_mont), d_table,
                                              r_f, r_p, chain_min_n, s);
    return hipGetLastError();
  });
}
// a^depth leaves -> the inner nodes, level by level, the root last: one hash launch per level of more than `tail` nodes (at
// most POSEIDON_MERKLE_TAIL_MAX), then one workgroup for all the levels that are left
hipError_t poseidon_merkle_launch(uint32_t width, const void* d_leaves, uint32_t depth, void* d_nodes, const uint64_t cap_mont[4],
                                  const void* d_table, uint32_t r_f, uint32_t r_p, uint32_t tail, size_t chain_min_n, hipStream_t s) {
  return by_width(width, [&](auto t) {
    constexpr int T = decltype(t)::value;
    constexpr uint32_t ARITY = T - 1, LG = merkle_lg(T);
    if (depth == 0 || LG * depth > 30 || tail == 0 || tail > POSEIDON_MERKLE_TAIL_MAX) return hipErrorInvalidValue;
    const Fe29<FS> cap = poseidon_capacity(cap_mont);
    const U128* in = (const U128*)d_leaves;
    U128* out = (U128*)d_nodes;
    size_t w = merkle_pow(LG, depth - 1);            // nodes of the level being written
    for (; w > tail; w /= ARITY) {                   // one launch per level; what is left is a power of the arity <= tail
      poseidon_hash_enqueue<T>(in, ARITY, ARITY, w, out, cap, d_table, r_f, r_p, chain_min_n, s);
      in = out;
      out += 2 * w;
    }
    hipLaunchKernelGGL((poseidon_merkle_tail_kernel<FS, T>), dim3(1), dim3(POSEIDON_THREADS), 0, s, in, out, (uint32_t)w, cap,
                       (const Fe29<FS>*)d_table, r_f, r_p);
    return hipGetLastError();
  });
}
hipError_t poseidon_paths_launch(uint32_t width, const void* d_leaves, const void* d_nodes, uint32_t depth, const void* d_indices, size_t n,
                                 void* d_paths, void* d_status, hipStream_t s) {
  return by_width(width, [&](auto t) {
    constexpr uint32_t LG = merkle_lg(decltype(t)::value);
    if (depth == 0 || LG * depth > 30) return hipErrorInvalidValue;
    hipLaunchKernelGGL(poseidon_merkle_paths_kernel, dim3(poseidon_grid(n * depth * (width - 2))), dim3(POSEIDON_THREADS), 0, s,
                       (const U128*)d_leaves, (const U128*)d_nodes, LG, depth, (const uint32_t*)d_indices, n, (U128*)d_paths,
                       (uint32_t*)d_status);
    return hipGetLastError();
  });
}
hipError_t poseidon_verify_launch(uint32_t width, const void* d_leaf_values, const void* d_indices, const void* d_paths, uint32_t depth,
                                  size_t n, const void* d_root, void* d_roots_out, void* d_status, const uint64_t cap_mont[4],
                                  const void* d_table, uint32_t r_f, uint32_t r_p, size_t quad_max, hipStream_t s) {
  return by_width(width, [&](auto t) {
    constexpr int T = decltype(t)::value;
    if (depth == 0 || merkle_lg(T) * depth > 30) return hipErrorInvalidValue;
    const Fe29<FS> cap = poseidon_capacity(cap_mont);
    if constexpr (T == 3) {   // the binary walker: a kernel of its own (h2_poseidon_merkle.hpp says why), on a quad or a lane
      if (n < quad_max)
        hipLaunchKernelGGL((poseidon_merkle_verify2_kernel<FS, true>), dim3(poseidon_grid(n, 4)), dim3(POSEIDON_THREADS), 0, s,
                           (const U128*)d_leaf_values, (const uint32_t*)d_indices, (const U128*)d_paths, depth, n, (const U128*)d_root,
                           (U128*)d_roots_out, (uint32_t*)d_status, cap, (const Fe29<FS>*)d_table, r_f, r_p);
      else
        hipLaunchKernelGGL((poseidon_merkle_verify2_kernel<FS, false>), dim3(poseidon_grid(n)), dim3(POSEIDON_THREADS), 0, s,
                           (const U128*)d_leaf_values, (const uint32_t*)d_indices, (const U128*)d_paths, depth, n, (const U128*)d_root,
                           (U128*)d_roots_out, (uint32_t*)d_status, cap, (const Fe29<FS>*)d_table, r_f, r_p);
    } else {
      hipLaunchKernelGGL((poseidon_merkle_verify_kernel<FS, T>), dim3(poseidon_grid(n)), dim3(POSEIDON_THREADS), 0, s,
                         (const U128*)d_leaf_values, (const uint32_t*)d_indices, (const U128*)d_paths, depth, n, (const U128*)d_root,
                         (U128*)d_roots_out, (uint32_t*)d_status, cap, (const Fe29<FS>*)d_table, r_f, r_p);
    }
    return hipGetLastError();
  });
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
size_t poseidon_update_scratch(size_t n, uint32_t depth) {
  MerkleUpdateScratch w;
  return merkle_update_scratch(n, depth, &w) == hipSuccess ? w.total : 0;
}
hipError_t poseidon_update_launch(void* d_leaves, void* d_nodes, uint32_t depth, const void* d_indices, const void* d_values, size_t n,
                                  void* d_status, const uint64_t cap2_mont[4], const void* d_table, uint32_t r_f, uint32_t r_p,
                                  size_t quad_max, void* d_scratch, size_t scratch_bytes, hipStream_t s) {
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
  hipLaunchKernelGGL(poseidon_merkle_update_keys_kernel<FS>, dim3(poseidon_grid(n)), dim3(POSEIDON_THREADS), 0, s,
                     (const uint32_t*)d_indices, (const U128*)d_values, n, depth, keys, pos, (uint32_t*)d_status);
  // stable, on the bits a leaf index has and the one above them: MERKLE_NO_KEY ends up behind every index
  if (hipError_t e = rocprim::radix_sort_pairs((char*)d_scratch + w.off_sort, w.sort_bytes, (const uint32_t*)keys, keys_sorted,
                                               (const uint32_t*)pos, pos_sorted, n, 0, depth + 1, s);
      e != hipSuccess)
    return e;
  hipLaunchKernelGGL(poseidon_merkle_update_leaves_kernel, dim3(poseidon_grid(n)), dim3(POSEIDON_THREADS), 0, s,
                     (const uint32_t*)keys_sorted, (const uint32_t*)pos_sorted, n, (const U128*)d_values, leaves, (uint32_t*)d_status);
  const bool quad_top = quad_max > 0;
  const uint32_t top = quad_top ? POSEIDON_TOP_QUAD : POSEIDON_TOP_LANE;
  uint32_t l = 0;
  for (; ((uint32_t)1 << (depth - 1 - l)) > top; l++) {
    const size_t width = (size_t)1 << (depth - 1 - l);
    const bool by_node = width <= n;
    const size_t items = by_node ? width : n;
    const U128* below = l == 0 ? leaves : nodes + 2 * merkle_level_offset(1, depth, l - 1);
    U128* level = nodes + 2 * merkle_level_offset(1, depth, l);
    if (items < quad_max)
      hipLaunchKernelGGL((poseidon_merkle_level_kernel<FS, true>), dim3(poseidon_grid(items, 4)), dim3(POSEIDON_THREADS), 0, s,
                         (const uint32_t*)keys_sorted, n, l, items, by_node, below, level, cap2, table, r_f, r_p);
    else
      hipLaunchKernelGGL((poseidon_merkle_level_kernel<FS, false>), dim3(poseidon_grid(items)), dim3(POSEIDON_THREADS), 0, s,
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
// host: poseidon_permute / poseidon_hash on a host copy of the table.  The sponge runs the width's own form only
template <int T, bool SPARSE>
hipError_t poseidon_selftest_t(int op, uint32_t len, uint32_t r_f, uint32_t r_p, const int32_t* table, const uint64_t* cap_mont,
                               const uint64_t* in, uint64_t* out) {
  const Fe29<FS>* tb = (const Fe29<FS>*)table;
  if (op == 0) {
    Fe29<FS> st[T];
    for (int j = 0; j < T; j++) {
      Fe<FS> a;
      memcpy(a.v, in + 4 * j, 32);
      st[j] = fe29_from_api(a);
    }
    poseidon_permute<FS, T, Fe29Compiler, SPARSE>(st, tb, r_f, r_p);
    for (int j = 0; j < T; j++) {
      const Fe<FS> r = fe29_to_api(st[j]);
      memcpy(out + 4 * j, r.v, 32);
    }
    return hipSuccess;
  }
  if (op == 1 && len >= 1 && SPARSE == POSEIDON_SPARSE<T>) {
    const Fe<FS> r = fe29_to_api(poseidon_hash<FS, T>((const U128*)in, len, poseidon_capacity(cap_mont), tb, r_f, r_p));
    memcpy(out, r.v, 32);
    return hipSuccess;
  }
  return hipErrorInvalidValue;
}
int poseidon_selftest(uint32_t width, int form, int op, uint32_t len, uint32_t r_f, uint32_t r_p, const int32_t* table,
                      const uint64_t* cap_mont, const uint64_t* in, uint64_t* out) {
  if (form < 0 || form > 2) return -1;
  const hipError_t e = by_width(width, [&](auto t) {
    constexpr int T = decltype(t)::value;
    if constexpr (T != 3) {
      if (poseidon_sparse<T>(form)) return poseidon_selftest_t<T, true>(op, len, r_f, r_p, table, cap_mont, in, out);
    }
    return poseidon_selftest_t<T, false>(op, len, r_f, r_p, table, cap_mont, in, out);
  });
  return e == hipSuccess ? 0 : -1;
}

const PoseidonOps OPS = {poseidon_table,        poseidon_permute_launch, poseidon_hash_launch,   poseidon_merkle_launch, poseidon_paths_launch,
                         poseidon_verify_launch, poseidon_update_scratch, poseidon_update_launch, poseidon_selftest};

}  // namespace

#if H2_CURVE_ID == 0
const PoseidonOps* poseidon_ops_bn254() { return &OPS; }
#elif H2_CURVE_ID == 1
const PoseidonOps* poseidon_ops_pallas() { return &OPS; }
#else
const PoseidonOps* poseidon_ops_vesta() { return &OPS; }
#endif

}  // namespace h2
