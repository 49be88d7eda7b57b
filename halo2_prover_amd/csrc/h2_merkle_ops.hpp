// h2_merkle_ops.hpp -- what the host side of h2_poseidon_merkle_{paths,verify,update}_device needs of the resident-tree
// kernels (h2_poseidon_quad.hpp): the status words and the launchers of one scalar field.  No kernels here.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace h2 {

// status words of the three calls (include/h2hip.h states the same values)
constexpr uint32_t MERKLE_OK = 0, MERKLE_RANGE = 1, MERKLE_NONCANONICAL = 2, MERKLE_SUPERSEDED = 3, MERKLE_MISMATCH = 4;
constexpr uint32_t MERKLE_NO_KEY = 0xFFFFFFFFu;      // sort key of a dropped update item: behind every leaf index (depth <= 30)

// The launchers of one scalar field (h2_merkle_impl.hip, a translation unit per curve).  d_leaves 2^depth elements, d_nodes
// poseidon_merkle's 2^depth - 1, indices u32, one u32 status per item.  quad_max: a launch of fewer hashes than this runs one
// permutation on four lanes, the others on one (0: never, SIZE_MAX: always).  update_scratch: the bytes d_scratch must hold
// for n items (host only, 0 when the sort cannot say); update sorts (index, position), stores the last value of every index
// and hashes the nodes above the stored leaves again, level by level.  cap2_mont = 2 2^64 as Montgomery limbs
struct MerkleOps {
  hipError_t (*paths)(const void* d_leaves, const void* d_nodes, uint32_t depth, const void* d_indices, size_t n, void* d_paths,
                      void* d_status, hipStream_t s);
  hipError_t (*verify)(const void* d_leaf_values, const void* d_indices, const void* d_paths, uint32_t depth, size_t n, const void* d_root,
                       void* d_roots_out, void* d_status, const uint64_t cap2_mont[4], const void* d_table, uint32_t r_f, uint32_t r_p,
                       size_t quad_max, hipStream_t s);
  size_t (*update_scratch)(size_t n, uint32_t depth);
  hipError_t (*update)(void* d_leaves, void* d_nodes, uint32_t depth, const void* d_indices, const void* d_values, size_t n,
                       void* d_status, const uint64_t cap2_mont[4], const void* d_table, uint32_t r_f, uint32_t r_p, size_t quad_max,
                       void* d_scratch, size_t scratch_bytes, hipStream_t s);
};
// The wide family (h2_poseidon_wide.hpp; the same translation units): width 5 or 9, arity a = width - 1.  d_table: (r_f +
// r_p) x width round constants, the width x width MDS and the sparse part (poseidon_wide_table_elems), in the working form.  cap_mont = len 2^64 (hash) or a 2^64
// (merkle, verify) as Montgomery limbs.  merkle: levels of more than `tail` nodes one hash launch each, the rest in one
// launch of one workgroup; hash and merkle take the single-chain products from chain_min_n lanes on, as the width-3 calls do.
// permute's form: 0 = the width's own (POSEIDON_WIDE_SPARSE), 1 = dense partial rounds, 2 = sparse; every other launch runs the
// width's own form.  A width that is not instantiated is hipErrorInvalidValue
struct PoseidonWideOps {
  hipError_t (*permute)(uint32_t width, int form, const void* d_in, void* d_out, size_t n, const void* d_table, uint32_t r_f,
                        uint32_t r_p, hipStream_t s);
  hipError_t (*hash)(uint32_t width, const void* d_msgs, uint32_t len, size_t msg_stride, size_t n, void* d_out,
                     const uint64_t cap_mont[4], const void* d_table, uint32_t r_f, uint32_t r_p, size_t chain_min_n, hipStream_t s);
  hipError_t (*merkle)(uint32_t width, const void* d_leaves, uint32_t depth, void* d_nodes, const uint64_t cap_mont[4],
                       const void* d_table, uint32_t r_f, uint32_t r_p, uint32_t tail, size_t chain_min_n, hipStream_t s);
  hipError_t (*paths)(uint32_t width, const void* d_leaves, const void* d_nodes, uint32_t depth, const void* d_indices, size_t n,
                      void* d_paths, void* d_status, hipStream_t s);
  hipError_t (*verify)(uint32_t width, const void* d_leaf_values, const void* d_indices, const void* d_paths, uint32_t depth, size_t n,
                       const void* d_root, void* d_roots_out, void* d_status, const uint64_t cap_mont[4], const void* d_table,
                       uint32_t r_f, uint32_t r_p, hipStream_t s);
  // host: the same templates on a host copy of the table; op 0 permutes one state of `width` elements, op 1 is
  // ConstantLength<len> of len elements; form as permute's
  int (*selftest)(uint32_t width, int form, int op, uint32_t len, uint32_t r_f, uint32_t r_p, const int32_t* table, const uint64_t* cap_mont,
                  const uint64_t* in, uint64_t* out);
};
const PoseidonWideOps* poseidon_wide_ops_bn254();
const PoseidonWideOps* poseidon_wide_ops_pallas();
const PoseidonWideOps* poseidon_wide_ops_vesta();

const MerkleOps* merkle_ops_bn254();
const MerkleOps* merkle_ops_pallas();
const MerkleOps* merkle_ops_vesta();

}  // namespace h2
