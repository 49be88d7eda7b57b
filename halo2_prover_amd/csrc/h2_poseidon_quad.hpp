// h2_poseidon_quad.hpp -- the Poseidon permutation of h2_poseidon.hpp with ONE PERMUTATION OVER THE FOUR LANES OF A DPP
// QUAD, and what runs on it: the walker that checks Merkle membership paths, the gather that cuts them and the in-place
// update of a resident tree (h2_poseidon_merkle_{paths,verify,update}_device).  Device only.
//
// Why.  A Merkle path is a chain of `depth` dependent hashes, and one hash on one lane is a chain of dependent products:
// a full round is 3 (S-box) x 3 words + 9 (MDS) = 18 products one after the other, a partial round 12, 816 in all for
// (8, 56), 864 for (8, 60).  Nothing a lane-per-path walker does can be shorter than depth x that.  The three words of a
// round are independent up to the MDS product, and so are its three rows:
//     lane q < 3 of a quad holds state word q
//     x   = fe29_norm(s + rc[q])             poseidon_add_rc on the lane's own word
//     y   = x^5                              three dependent products (partial round: lanes 1, 2 keep x -- quad_pick)
//     s   = m[q][0] y_0 + m[q][1] y_1 + m[q][2] y_2        y_j broadcast with quad_bcast (v_mov_b32 quad_perm, no LDS);
//                                            three independent products and two additions, the sum left un-normalised
// The dependent chain of a round is 4 products deep whatever the round's kind, (r_f + r_p) x 4 = 256 or 272 for a
// permutation.  Full and partial rounds are ONE instruction stream: a partial round computes the S-box on every lane and
// drops the result on lanes 1..3.  Lane 3 idles: it carries lane 2's word and constants, its result is never read.  A
// quad spends 4 x 272 lane-products where a lane spends 864, so where the device is full the lane form does more hashes
// per second; which form a launch takes is decided by size (POSEIDON_WALK_QUAD_MAX in h2_poseidon.hpp).
//
// Bounds.  The analysis at the top of h2_poseidon.hpp carries over word for word, because every word sees the same
// operations in the same order on the same integers: s + rc normalised once (limbs <= 4 (2^29 - 1) before, carries <= 3),
// fe29_sqr / fe29_sqr / fe29_mul on normalised operands, fe29_mul(y, m) with m canonical on the narrow side, three
// products summed without a carry pass, |s| < 3.1 p.  In a partial round lanes 1 and 2 pass the normalised x (|x| < c p,
// c = 4.1) exactly as the lane form does; the S-box they compute beside it is within fe29_sqr's and fe29_mul's bounds
// like any full round's and is dropped.  A broadcast moves limbs, it changes none.  The walker feeds the permutation
// fe29_from_api of a canonical element (canonical, normalised), the normalised word 0 of the previous level and the
// capacity word: the c = 5.1 case of that analysis does not even arise (nothing is added to a word before round 0).
// An element that is NOT canonical never reaches a product: the walker stops at it with status 2.
//
// Constants.  Round constant and MDS row differ per lane, so they cannot all come through the scalar cache as in the lane
// form.  Chosen: plain vector loads from the same table in HBM (36-byte entries, lane q reads entry 3 r + q).
//   MDS row    three entries, loaded once per permutation and KEPT IN REGISTERS: 27 VGPRs.
//   rc         one entry per round: 9 VGPRs, and the load of round r + 1's is issued at the top of round r, so its
//              latency (L2 after the first quad of a launch has touched the 7 KB table) hides under four products.
//              The last round's prefetch reads the table's first MDS entry, which is there: no branch.
// LDS is not used: a copy of the table per workgroup would cost a barrier and 7 KB per launch for loads that are already
// off the critical path.  Registers (hipcc --save-temps, gfx950; vgpr / sgpr / scratch bytes):
//     kernel                             BN254 (8, 60)       Pallas, Vesta (8, 56)
//     poseidon_merkle_verify_kernel      116 / 106 / 0       109 / 90 / 0         quad form
//                                         98 / 106 / 0        91 / 106 / 0        lane form
//     poseidon_merkle_level_kernel        98 / 87 / 0        100 / 72 / 0         quad
//                                         79 / 106 / 0        79 / 98 / 0         lane
//     poseidon_merkle_top_kernel         100 / 81 / 0        102 / 68 / 0         quad
//                                         81 / 106 / 0        81 / 94 / 0         lane
// No scratch anywhere.  The quad forms hold 18 - 21 VGPRs more than the lane forms -- the 27 of the MDS row and the 9 of
// the prefetched constant against the lane form's three state words -- and a third of the code (15 - 19 KB against 49 -
// 62 KB: six inlined products in one round body where the lane form has thirty in two).  Four waves per SIMD fit (the lane
// forms: four to six); a launch that is latency-bound has one.  profiles/poseidon_merkle_resources.txt has every kernel.
#pragma once
#include "h2_curve_quad.hpp"
#include "h2_merkle_ops.hpp"
#include "h2_poseidon.hpp"

namespace h2 {

// The update's single-workgroup top: levels of at most this many nodes.  256 threads are 64 quads or 256 lanes
constexpr uint32_t POSEIDON_TOP_QUAD = 64, POSEIDON_TOP_LANE = 256;

// first node of level l (l = 0: the leaves' parents) in the node array of a tree of 2^depth leaves
H2_HD constexpr size_t merkle_level_offset(uint32_t depth, uint32_t l) { return ((size_t)1 << depth) - ((size_t)1 << (depth - l)); }

#if defined(__HIPCC__)
// s: the lane's word of the state (lane q < 3 of the quad: word q; lane 3: anything within word 2's bounds), normalised or
// a sum of three products -> the lane's word of the permuted state, normalised.  All four lanes of the quad are active
template <class FS, class A = Fe29Compiler>
__device__ __forceinline__ Fe29<FS> poseidon_permute_quad(Fe29<FS> s, const Fe29<FS>* __restrict__ table, uint32_t r_f, uint32_t r_p) {
  const uint32_t q = threadIdx.x & 3, w = q < 3 ? q : 2;
  const uint32_t others = 0u - (uint32_t)(q != 0);
  const uint32_t rounds = r_f + r_p, half = r_f >> 1;
  const Fe29<FS>* const row = table + 3 * (size_t)rounds + 3 * w;
  const Fe29<FS> m0 = row[0], m1 = row[1], m2 = row[2];
  const Fe29<FS>* rc = table + w;
  Fe29<FS> c = *rc;
#pragma unroll 1
  for (uint32_t r = 0; r < rounds; r++) {
    const Fe29<FS> x = fe29_norm(fe29_add(s, c));
    rc += 3;
    c = *rc;                                         // the next round's; behind the last round: an MDS entry, not used
    const uint32_t keep = r - half < r_p ? others : 0u;   // a partial round: lanes 1.. pass x
    const Fe29<FS> y = quad_pick(keep, x, poseidon_pow5<FS, A>(x));
    s = fe29_add(fe29_add(A::template mul<FS>(quad_bcast<0>(y), m0), A::template mul<FS>(quad_bcast<1>(y), m1)),
                 A::template mul<FS>(quad_bcast<2>(y), m2));
  }
  return fe29_norm(s);
}
// ConstantLength<2> of (a, b), all three replicated across the quad -> the hash, normalised, replicated
template <class FS>
__device__ __forceinline__ Fe29<FS> poseidon_hash2_quad(const Fe29<FS>& a, const Fe29<FS>& b, const Fe29<FS>& cap2,
                                                        const Fe29<FS>* __restrict__ table, uint32_t r_f, uint32_t r_p) {
  const uint32_t q = threadIdx.x & 3;
  const Fe29<FS> word = quad_pick(0u - (uint32_t)(q == 0), a, quad_pick(0u - (uint32_t)(q == 1), b, cap2));
  return quad_bcast<0>(poseidon_permute_quad<FS>(word, table, r_f, r_p));
}
// either form behind one name.  QUAD: four lanes per hash, operands and result replicated
template <class FS, bool QUAD>
__device__ __forceinline__ Fe29<FS> merkle_hash2(const Fe29<FS>& a, const Fe29<FS>& b, const Fe29<FS>& cap2,
                                                 const Fe29<FS>* __restrict__ table, uint32_t r_f, uint32_t r_p) {
  if constexpr (QUAD) return poseidon_hash2_quad<FS>(a, b, cap2, table, r_f, r_p);
  else return poseidon_hash2<FS, Fe29Compiler>(a, b, cap2, table, r_f, r_p);
}

// ---- paths: a gather ----------------------------------------------------------------------------------------------------
// one lane per (item, level): paths[i][l] = the sibling of leaf indices[i]'s ancestor at level l, or zero when the index is
// out of range.  The index is checked against 2^depth before it addresses anything
static __global__ void __launch_bounds__(POSEIDON_THREADS)
poseidon_merkle_paths_kernel(const U128* __restrict__ leaves, const U128* __restrict__ nodes, uint32_t depth,
                             const uint32_t* __restrict__ indices, size_t n, U128* __restrict__ paths, uint32_t* __restrict__ status) {
  const size_t stride = (size_t)gridDim.x * POSEIDON_THREADS, total = n * depth;
  for (size_t t = (size_t)blockIdx.x * POSEIDON_THREADS + threadIdx.x; t < total; t += stride) {
    const size_t i = t / depth;
    const uint32_t l = (uint32_t)(t - i * depth), idx = indices[i];
    const bool ok = idx < (1u << depth);
    U128 lo = U128{0, 0, 0, 0}, hi = lo;
    if (ok) {
      const size_t sib = (size_t)((idx >> l) ^ 1u);
      const U128* src = l == 0 ? leaves + 2 * sib : nodes + 2 * (merkle_level_offset(depth, l - 1) + sib);
      lo = src[0];
      hi = src[1];
    }
    paths[2 * t] = lo;
    paths[2 * t + 1] = hi;
    if (l == 0) status[i] = ok ? MERKLE_OK : MERKLE_RANGE;
  }
}

// ---- verify: one quad (or one lane) per path ----------------------------------------------------------------------------
// cur = leaf; per level cur = H(sib, cur) if the index bit is set, else H(cur, sib); the value stays in the working form
// between levels.  An index out of range (status 1) or an element that is not canonical (status 2) ends the item with a
// zero root before any product sees it.  root: null, or the element every computed root is compared with
template <class FS, bool QUAD>
__global__ void __launch_bounds__(POSEIDON_THREADS)
poseidon_merkle_verify_kernel(const U128* __restrict__ leaf_values, const uint32_t* __restrict__ indices, const U128* __restrict__ paths,
                              uint32_t depth, size_t n, const U128* __restrict__ root, U128* __restrict__ roots_out,
                              uint32_t* __restrict__ status, Fe29<FS> cap2, const Fe29<FS>* __restrict__ table, uint32_t r_f,
                              uint32_t r_p) {
  constexpr uint32_t LANES = QUAD ? 4 : 1;
  const size_t stride = (size_t)gridDim.x * (POSEIDON_THREADS / LANES);
  for (size_t i = ((size_t)blockIdx.x * POSEIDON_THREADS + threadIdx.x) / LANES; i < n; i += stride) {
    const uint32_t idx = indices[i];
    const Fe<FS> leaf = fe_load<FS>(leaf_values + 2 * i);
    uint32_t st = idx < (1u << depth) ? MERKLE_OK : MERKLE_RANGE;
    if (st == MERKLE_OK && !fe_is_canonical(leaf)) st = MERKLE_NONCANONICAL;
    Fe29<FS> cur = fe29_from_api(leaf);
    const U128* path = paths + 2 * i * depth;
#pragma unroll 1
    for (uint32_t l = 0; l < depth && st == MERKLE_OK; l++) {
      const Fe<FS> sib = fe_load<FS>(path + 2 * (size_t)l);
      if (!fe_is_canonical(sib)) {
        st = MERKLE_NONCANONICAL;
        break;
      }
      const Fe29<FS> s = fe29_from_api(sib);
      const uint32_t right = 0u - ((idx >> l) & 1u);
      cur = merkle_hash2<FS, QUAD>(quad_pick(right, s, cur), quad_pick(right, cur, s), cap2, table, r_f, r_p);
    }
    Fe<FS> r;
#pragma unroll
    for (int j = 0; j < 8; j++) r.v[j] = 0;
    if (st == MERKLE_OK) {
      r = fe29_to_api(cur);
      if (root) {
        const Fe<FS> want = fe_load<FS>(root);
        uint32_t diff = 0;
#pragma unroll
        for (int j = 0; j < 8; j++) diff |= r.v[j] ^ want.v[j];
        if (diff) st = MERKLE_MISMATCH;
      }
    }
    if (!QUAD || (threadIdx.x & 3) == 0) {
      if (roots_out) fe_store<FS>(roots_out + 2 * i, r);
      status[i] = st;
    }
  }
}

// ---- update ---------------------------------------------------------------------------------------------------------------
// 1. keys: item i -> (key, position).  key = the index, or MERKLE_NO_KEY for an item that is dropped (status 1: index out of
//    range; status 2: value not canonical).  2. a stable sort by key (the launcher's): the items of one leaf stand together in
//    array order, the dropped ones behind everything.  3. leaves: the LAST of a run stores its value, the others get status
//    3.  4. level by level, only the nodes above a stored leaf are hashed again -- found from the sorted keys alone, by
//    comparing neighbours (a launch over items) or by a binary search per node (a launch over nodes, and the top).
template <class FS>
__global__ void __launch_bounds__(POSEIDON_THREADS)
poseidon_merkle_update_keys_kernel(const uint32_t* __restrict__ indices, const U128* __restrict__ values, size_t n, uint32_t depth,
                                   uint32_t* __restrict__ keys, uint32_t* __restrict__ pos, uint32_t* __restrict__ status) {
  const size_t stride = (size_t)gridDim.x * POSEIDON_THREADS;
  for (size_t i = (size_t)blockIdx.x * POSEIDON_THREADS + threadIdx.x; i < n; i += stride) {
    const uint32_t idx = indices[i];
    uint32_t st = idx < (1u << depth) ? MERKLE_OK : MERKLE_RANGE;
    if (st == MERKLE_OK && !fe_is_canonical(fe_load<FS>(values + 2 * i))) st = MERKLE_NONCANONICAL;
    keys[i] = st == MERKLE_OK ? idx : MERKLE_NO_KEY;
    pos[i] = (uint32_t)i;
    status[i] = st;
  }
}
// keys / pos: sorted.  A key below 2^depth was checked by the keys kernel; nothing else addresses the leaves
static __global__ void __launch_bounds__(POSEIDON_THREADS)
poseidon_merkle_update_leaves_kernel(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ pos, size_t n,
                                     const U128* __restrict__ values, U128* __restrict__ leaves, uint32_t* __restrict__ status) {
  const size_t stride = (size_t)gridDim.x * POSEIDON_THREADS;
  for (size_t j = (size_t)blockIdx.x * POSEIDON_THREADS + threadIdx.x; j < n; j += stride) {
    const uint32_t k = keys[j];
    if (k == MERKLE_NO_KEY) continue;
    const size_t p = pos[j];
    if (j + 1 < n && keys[j + 1] == k) {
      status[p] = MERKLE_SUPERSEDED;
    } else {
      leaves[2 * (size_t)k] = values[2 * p];
      leaves[2 * (size_t)k + 1] = values[2 * p + 1];
    }
  }
}
// does a stored leaf lie below node t of level l?  The leaves below it are [t << (l + 1), (t + 1) << (l + 1)): the first
// sorted key that is not below the range's start decides (MERKLE_NO_KEY is above every range)
__device__ __forceinline__ bool merkle_node_touched(const uint32_t* __restrict__ keys, size_t n, uint32_t l, uint32_t t) {
  const uint32_t first = t << (l + 1), last = first + ((1u << (l + 1)) - 1);
  size_t lo = 0, hi = n;                         // lo <= hi <= n throughout
  while (lo < hi) {
    const size_t mid = lo + ((hi - lo) >> 1);
    if (keys[mid] < first) lo = mid + 1;
    else hi = mid;
  }
  return lo < n && keys[lo] <= last;
}
// node `node` of level l from its two children at `below` (the leaves, or level l - 1), written in the API form
template <class FS, bool QUAD>
__device__ __forceinline__ void merkle_rehash(const U128* below, U128* level, uint32_t node, const Fe29<FS>& cap2,
                                              const Fe29<FS>* __restrict__ table, uint32_t r_f, uint32_t r_p) {
  const Fe29<FS> a = fe29_from_api(fe_load<FS>(below + 4 * (size_t)node));
  const Fe29<FS> b = fe29_from_api(fe_load<FS>(below + 4 * (size_t)node + 2));
  const Fe<FS> h = fe29_to_api(merkle_hash2<FS, QUAD>(a, b, cap2, table, r_f, r_p));
  if (!QUAD || (threadIdx.x & 3) == 0) fe_store<FS>(level + 2 * (size_t)node, h);
}
// One level, `items` hashes at most.  by_node: item t is node t of the level (items = its width), hashed when a stored leaf
// lies below it.  Otherwise item j is sorted key j (items = n), which hashes node key >> (l + 1) when it is the first of the
// keys below that node.  `below` is not written by this launch and `level` not read: they are different levels
template <class FS, bool QUAD>
__global__ void __launch_bounds__(POSEIDON_THREADS)
poseidon_merkle_level_kernel(const uint32_t* __restrict__ keys, size_t n, uint32_t l, size_t items, bool by_node, const U128* below,
                             U128* level, Fe29<FS> cap2, const Fe29<FS>* __restrict__ table, uint32_t r_f, uint32_t r_p) {
  constexpr uint32_t LANES = QUAD ? 4 : 1;
  const size_t stride = (size_t)gridDim.x * (POSEIDON_THREADS / LANES);
  for (size_t j = ((size_t)blockIdx.x * POSEIDON_THREADS + threadIdx.x) / LANES; j < items; j += stride) {
    uint32_t node;
    if (by_node) {
      node = (uint32_t)j;
      if (!merkle_node_touched(keys, n, l, node)) continue;
    } else {
      const uint32_t k = keys[j];
      node = k >> (l + 1);
      if (k == MERKLE_NO_KEY || (j > 0 && (keys[j - 1] >> (l + 1)) == node)) continue;
    }
    merkle_rehash<FS, QUAD>(below, level, node, cap2, table, r_f, r_p);
  }
}
// The top of the tree in ONE workgroup: level l0 (at most POSEIDON_TOP_QUAD / POSEIDON_TOP_LANE nodes) and every level
// above it.  A level's stores and the next level's loads of them are separated by a barrier, which orders global memory
// within the workgroup; every thread reaches every barrier.  leaves is read only when l0 = 0
template <class FS, bool QUAD>
__global__ void __launch_bounds__(POSEIDON_THREADS)
poseidon_merkle_top_kernel(const uint32_t* __restrict__ keys, size_t n, uint32_t depth, uint32_t l0, const U128* leaves, U128* nodes,
                           Fe29<FS> cap2, const Fe29<FS>* __restrict__ table, uint32_t r_f, uint32_t r_p) {
  const uint32_t t = QUAD ? threadIdx.x >> 2 : threadIdx.x;
#pragma unroll 1
  for (uint32_t l = l0; l < depth; l++) {
    const uint32_t width = 1u << (depth - 1 - l);
    const U128* below = l == 0 ? leaves : nodes + 2 * merkle_level_offset(depth, l - 1);
    if (t < width && merkle_node_touched(keys, n, l, t))
      merkle_rehash<FS, QUAD>(below, nodes + 2 * merkle_level_offset(depth, l), t, cap2, table, r_f, r_p);
    __threadfence_block();
    __syncthreads();
  }
}
#endif  // __HIPCC__

}  // namespace h2
