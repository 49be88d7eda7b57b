// h2_poseidon_ops.hpp -- what the host side of h2_poseidon_* needs of the Poseidon kernels (h2_poseidon.hpp,
// h2_poseidon_merkle.hpp): the status words and the launchers of one scalar field.  No kernels here.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace h2 {

// status words of the paths, verify and update calls (include/h2hip.h states the same values)
constexpr uint32_t MERKLE_OK = 0, MERKLE_RANGE = 1, MERKLE_NONCANONICAL = 2, MERKLE_SUPERSEDED = 3, MERKLE_MISMATCH = 4;
constexpr uint32_t MERKLE_NO_KEY = 0xFFFFFFFFu;      // sort key of a dropped update item: behind every leaf index (depth <= 30)

// The launchers of one scalar field (h2_poseidon_impl.hip, a translation unit per curve).  width 3, 5 or 9, arity a =
// width - 1; a width that is not instantiated is hipErrorInvalidValue.  d_table: poseidon_table_elems entries in the working
// form, as `table` (host) makes them from n constants as Montgomery limbs.  cap_mont = len 2^64 (hash) or a 2^64 (merkle,
// verify, update) as Montgomery limbs.
//   permute   n states of `width` elements, d_out == d_in allowed.  form: the partial rounds, 0 = the width's own
//             (POSEIDON_SPARSE), 1 = dense, 2 = sparse; every other launch runs the width's own form, width 3 always the dense
//   hash      ConstantLength<len> of n messages msg_stride elements apart; a launch of chain_min_n lanes or more runs on the
//             single-chain products where the field has them (0: always, SIZE_MAX: never)
//   merkle    a^depth leaves -> the inner nodes, level by level, the root last: levels of more than `tail` nodes one hash
//             launch each, the rest in one launch of one workgroup
//   paths     d_leaves a^depth elements, d_nodes merkle's, indices u32, one u32 status per item
//   verify    quad_max: a width-3 launch of fewer paths than this runs one permutation on four lanes, the others on one (0:
//             never, SIZE_MAX: always)
//   update    binary trees.  update_scratch: the bytes d_scratch must hold for n items (host only, 0 when the sort cannot
//             say); update sorts (index, position), stores the last value of every index and hashes the nodes above the
//             stored leaves again, level by level, with quad_max as verify's
//   selftest  host: the same templates on a host copy of the table; op 0 permutes one state of `width` elements, op 1 is
//             ConstantLength<len> of len elements; form as permute's
struct PoseidonOps {
  void (*table)(const uint64_t* api, size_t n, int32_t* out);
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
                       uint32_t r_f, uint32_t r_p, size_t quad_max, hipStream_t s);
  size_t (*update_scratch)(size_t n, uint32_t depth);
  hipError_t (*update)(void* d_leaves, void* d_nodes, uint32_t depth, const void* d_indices, const void* d_values, size_t n,
                       void* d_status, const uint64_t cap2_mont[4], const void* d_table, uint32_t r_f, uint32_t r_p, size_t quad_max,
                       void* d_scratch, size_t scratch_bytes, hipStream_t s);
  int (*selftest)(uint32_t width, int form, int op, uint32_t len, uint32_t r_f, uint32_t r_p, const int32_t* table, const uint64_t* cap_mont,
                  const uint64_t* in, uint64_t* out);
};
const PoseidonOps* poseidon_ops_bn254();
const PoseidonOps* poseidon_ops_pallas();
const PoseidonOps* poseidon_ops_vesta();

}  // namespace h2
