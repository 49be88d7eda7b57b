// h2_poseidon_merkle.hpp -- Merkle trees of ConstantLength<a> Poseidon hashes, arity a = T - 1 = 2, 4, 8 (h2_poseidon.hpp):
// the single-workgroup tail of the tree build, the gather that cuts membership paths, the walker that checks them, and --
// binary trees only -- the in-place update of a resident tree (h2_poseidon_merkle_{paths,verify,update}_device and their
// h2_poseidon_wide_* forms).  At T = 3 the walker -- a kernel of its own, poseidon_merkle_verify2_kernel -- and the update also
// run on the quad permutation (h2_poseidon_quad.hpp).
//
// Registers of the width-3 walker and update (hipcc --save-temps, gfx950; vgpr / sgpr / scratch bytes):
//     kernel                             BN254 (8, 60)       Pallas, Vesta (8, 56)
//     poseidon_merkle_verify2_kernel     116 / 106 / 0       109 / 90 / 0         quad form
//                                         98 / 106 / 0        91 / 106 / 0        lane form
//     poseidon_merkle_level_kernel        98 / 87 / 0        100 / 72 / 0         quad
//                                         79 / 106 / 0        79 / 98 / 0         lane
//     poseidon_merkle_top_kernel         100 / 81 / 0        102 / 68 / 0         quad
//                                         81 / 106 / 0        81 / 94 / 0         lane
// No scratch anywhere.  The quad forms hold 18 - 21 VGPRs more than the lane forms -- the 27 of the MDS row and the 9 of
// the prefetched constant against the lane form's three state words -- and a third of the code (15 - 19 KB against 49 -
// 62 KB: six inlined products in one round body where the lane form has thirty in two).  Four waves per SIMD fit (the lane
// forms: four to six); a launch that is latency-bound has one.  profiles/poseidon_one_family_resources.txt has every kernel.
#pragma once
#include "h2_poseidon_ops.hpp"
#include "h2_poseidon_quad.hpp"

namespace h2 {

// The update's single-workgroup top: levels of at most this many nodes.  256 threads are 64 quads or 256 lanes
constexpr uint32_t POSEIDON_TOP_QUAD = 64, POSEIDON_TOP_LANE = 256;

#if defined(__HIPCC__)
// a node of a binary tree from its two children, in either form behind one name.  QUAD: four lanes per hash, operands and
// result replicated
template <class FS, bool QUAD>
__device__ __forceinline__ Fe29<FS> merkle_hash2(const Fe29<FS>& a, const Fe29<FS>& b, const Fe29<FS>& cap2,
                                                 const Fe29<FS>* __restrict__ table, uint32_t r_f, uint32_t r_p) {
  if constexpr (QUAD) {
    return poseidon_hash2_quad<FS>(a, b, cap2, table, r_f, r_p);
  } else {
    Fe29<FS> s[3] = {a, b, cap2};
    return poseidon_hash_words<FS, 3, Fe29Compiler>(s, cap2, table, r_f, r_p);
  }
}

// ---- the tail of the tree build ----------------------------------------------------------------------------------------
// The top of an a-ary tree (a = T - 1) in ONE workgroup: `width` nodes (a power of a, 1 <= width <=
// POSEIDON_MERKLE_TAIL_MAX) from their a width children at `in`, then every level above them up to the root, each level
// written behind the one before at `out`.  The levels above the first are read from LDS in the working form -- no
// conversion in, no trip through memory -- and a barrier separates a level's writes from the next level's reads; two
// buffers alternate, so a level never overwrites what another lane still reads.  Limb-major layout: lane i's limb l at
// [l][i], no bank conflict on the store and a-way on the stride-a loads.  The first level goes to lvl_a (up to TAIL_MAX
// nodes), the second to lvl_b (up to TAIL_MAX / a)
template <class FS, int T>
__global__ void __launch_bounds__(POSEIDON_THREADS)
poseidon_merkle_tail_kernel(const U128* __restrict__ in, U128* __restrict__ out, uint32_t width, Fe29<FS> cap,
                            const Fe29<FS>* __restrict__ table, uint32_t r_f, uint32_t r_p) {
  constexpr uint32_t ARITY = T - 1;
  __shared__ int32_t lvl_a[9 * POSEIDON_MERKLE_TAIL_MAX];
  __shared__ int32_t lvl_b[9 * (POSEIDON_MERKLE_TAIL_MAX / ARITY)];
  const uint32_t t = threadIdx.x;
  int32_t* src = lvl_b;
  int32_t* dst = lvl_a;
  uint32_t src_ld = POSEIDON_MERKLE_TAIL_MAX / ARITY, dst_ld = POSEIDON_MERKLE_TAIL_MAX;
  bool first = true;
#pragma unroll 1
  for (uint32_t w = width; w >= 1; w /= ARITY) {
    for (uint32_t i = t; i < w; i += POSEIDON_THREADS) {
      Fe29<FS> s[T];
      if (first) {
        poseidon_wide_each<0, T - 1>([&](auto c) { s[c] = fe29_from_api(fe_load<FS>(in + 2 * ((size_t)ARITY * i + c))); });
      } else {
        poseidon_wide_each<0, T - 1>([&](auto c) {
#pragma unroll
          for (int l = 0; l < 9; l++) s[c].v[l] = src[l * src_ld + ARITY * i + c];
        });
      }
      const Fe29<FS> h = poseidon_hash_words<FS, T, Fe29Compiler>(s, cap, table, r_f, r_p);
#pragma unroll
      for (int l = 0; l < 9; l++) dst[l * dst_ld + i] = h.v[l];
      fe_store<FS>(out + 2 * (size_t)i, fe29_to_api(h));
    }
    __syncthreads();
    out += 2 * (size_t)w;
    int32_t* const tp = src; src = dst; dst = tp;
    const uint32_t tl = src_ld; src_ld = dst_ld; dst_ld = tl;
    first = false;
  }
}

// ---- paths: a gather --------------------------------------------------------------------------------------------------
// one lane per (item, level, sibling): paths[i][l][k] = child c of the parent of leaf indices[i]'s ancestor at level l, c
// running over the parent's a = 2^lg children in order with the ancestor's own position left out (a binary tree: the one
// sibling (idx >> l) ^ 1); zero when the index is out of range.  The index is checked against a^depth before it addresses
// anything
static __global__ void __launch_bounds__(POSEIDON_THREADS)
poseidon_merkle_paths_kernel(const U128* __restrict__ leaves, const U128* __restrict__ nodes, uint32_t lg, uint32_t depth,
                             const uint32_t* __restrict__ indices, size_t n, U128* __restrict__ paths, uint32_t* __restrict__ status) {
  const uint32_t sibs = (1u << lg) - 1, per_item = depth * sibs;
  const size_t stride = (size_t)gridDim.x * POSEIDON_THREADS, total = n * per_item;
  for (size_t t = (size_t)blockIdx.x * POSEIDON_THREADS + threadIdx.x; t < total; t += stride) {
    const size_t i = t / per_item;
    const uint32_t e = (uint32_t)(t - i * per_item), l = e / sibs, k = e - l * sibs, idx = indices[i];
    const bool ok = idx < ((uint32_t)1 << (lg * depth));
    U128 lo = U128{0, 0, 0, 0}, hi = lo;
    if (ok) {
      const uint32_t node = idx >> (lg * l), pos = node & sibs;
      const size_t sib = (size_t)((node & ~sibs) | (k < pos ? k : k + 1));
      const U128* src = l == 0 ? leaves + 2 * sib : nodes + 2 * (merkle_level_offset(lg, depth, l - 1) + sib);
      lo = src[0];
      hi = src[1];
    }
    paths[2 * t] = lo;
    paths[2 * t + 1] = hi;
    if (e == 0) status[i] = ok ? MERKLE_OK : MERKLE_RANGE;
  }
}

// ---- verify --------------------------------------------------------------------------------------------------------------
// cur = leaf; per level the a words are the level's a - 1 siblings with cur inserted at its position, cur = their hash; the
// value stays in the working form between levels.  An index out of range (status 1) or an element that is not canonical
// (status 2) ends the item with a zero root before any product sees it.  root: null, or the element every computed root is
// compared with.
//
// The walker is TWO kernels, the one place where the family keeps a width apart.  Measured against the parent (profiles/
// poseidon_one_family_parent_vs_branch.txt): the general kernel below at T = 3 -- both child slots filled from sibling 0 by a
// load, a check and a select each -- ran 0.15 - 0.25 % behind the binary walker on both walk forms with all registers equal;
// with the single load and quad_pick put back inside it under `if constexpr (T == 3)` it ran 0.9 - 1.1 % (lane) and 0.4 %
// (quad) behind on the Pasta fields, one VGPR above the binary walker.  So the binary walker stays as it was written, one
// quad or one lane per path, and the general kernel serves the arities 4 and 8.
template <class FS, bool QUAD>
__global__ void __launch_bounds__(POSEIDON_THREADS)
poseidon_merkle_verify2_kernel(const U128* __restrict__ leaf_values, const uint32_t* __restrict__ indices, const U128* __restrict__ paths,
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
      const uint32_t right = 0u - ((idx >> l) & 1u);      // cur = H(sib, cur) if the index bit is set, else H(cur, sib)
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
// the arities 4 and 8 (T = 5, 9; the arithmetic is right at T = 3 too): one lane per path
template <class FS, int T>
__global__ void __launch_bounds__(POSEIDON_THREADS)
poseidon_merkle_verify_kernel(const U128* __restrict__ leaf_values, const uint32_t* __restrict__ indices, const U128* __restrict__ paths,
                              uint32_t depth, size_t n, const U128* __restrict__ root, U128* __restrict__ roots_out,
                              uint32_t* __restrict__ status, Fe29<FS> cap, const Fe29<FS>* __restrict__ table, uint32_t r_f,
                              uint32_t r_p) {
  constexpr uint32_t ARITY = T - 1, SIBS = ARITY - 1, LG = merkle_lg(T);
  static_assert(ARITY == (1u << LG), "arity 2, 4 or 8");
  const size_t stride = (size_t)gridDim.x * POSEIDON_THREADS;
  for (size_t i = (size_t)blockIdx.x * POSEIDON_THREADS + threadIdx.x; i < n; i += stride) {
    const uint32_t idx = indices[i];
    const Fe<FS> leaf = fe_load<FS>(leaf_values + 2 * i);
    uint32_t st = idx < ((uint32_t)1 << (LG * depth)) ? MERKLE_OK : MERKLE_RANGE;
    if (st == MERKLE_OK && !fe_is_canonical(leaf)) st = MERKLE_NONCANONICAL;
    Fe29<FS> cur = fe29_from_api(leaf);
    const U128* path = paths + 2 * i * depth * SIBS;
#pragma unroll 1
    for (uint32_t l = 0; l < depth && st == MERKLE_OK; l++) {
      const uint32_t pos = (idx >> (LG * l)) & SIBS;
      Fe29<FS> s[T];
      poseidon_wide_each<0, T - 1>([&](auto ci) {
        constexpr uint32_t c = (uint32_t)decltype(ci)::value;
        // child c: cur at its own position, else sibling c (before it) or c - 1 (behind it).  k <= SIBS - 1 either way: the
        // load that position `pos` does not need stays inside the level's siblings
        const uint32_t k = c < pos ? c : c == 0 ? 0 : c - 1;
        const Fe<FS> sib = fe_load<FS>(path + 2 * ((size_t)l * SIBS + k));
        if (c != pos && !fe_is_canonical(sib)) st = MERKLE_NONCANONICAL;
        s[c] = fe29_from_api(sib);
        if (c == pos) s[c] = cur;
      });
      if (st != MERKLE_OK) break;
      cur = poseidon_hash_words<FS, T, Fe29Compiler>(s, cap, table, r_f, r_p);
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
    if (roots_out) fe_store<FS>(roots_out + 2 * i, r);
    status[i] = st;
  }
}

// ---- update (binary trees) ------------------------------------------------------------------------------------------------
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
    const U128* below = l == 0 ? leaves : nodes + 2 * merkle_level_offset(1, depth, l - 1);
    if (t < width && merkle_node_touched(keys, n, l, t))
      merkle_rehash<FS, QUAD>(below, nodes + 2 * merkle_level_offset(1, depth, l), t, cap2, table, r_f, r_p);
    __threadfence_block();
    __syncthreads();
  }
}
#endif  // __HIPCC__

}  // namespace h2
