// h2_poseidon.hpp -- the Poseidon permutation (width 3, rate 2, S-box x^5), the ConstantLength sponge on it and a Merkle
// tree of ConstantLength<2> hashes, over the scalar field of a curve, on the 9 x 29-bit working form (h2_field29.hpp).
//
// Restates the reference's circuits/src/poseidon/primitives.rs:87-132 (permute: r_f / 2 full rounds, r_p partial rounds,
// r_f / 2 full rounds; a round = add the round constants, S-box, MDS product) and :204-390 (the ConstantLength<L> sponge:
// state (0, 0, L 2^64), the message absorbed two words at a time, zero-padded, one permutation per absorb, output =
// word 0).  The judge is oracle/pyref.py.  The constants come from h2_poseidon_host.hpp; the kernels read them from a table
// in HBM in the working form (x 2^261 mod p, canonical, nine limbs = 36 bytes each): (r_f + r_p) x 3 round constants, then
// the 3 x 3 MDS row-major.  The round index is the same in every lane, so the table is read through the scalar cache and
// the constants stay out of the vector registers.
//
// Bounds, against the invariants at the top of h2_field29.hpp.  Write rho = p / R' (R' = 2^261): rho = 2^-7 (1 + 2^-127)
// for the Pasta primes, below 2^-7 for BN254's.  fe29_mul(a, b) needs |a_i| < 2^30, |b_j| < 2^29 and returns a value in
// (a b / R' - p, a b / R'] with normalised limbs; fe29_sqr(a) needs |a_i| < 2^29 and a^2 <= 64 p^2.
//   state   Between rounds a state word s is the SUM OF THREE PRODUCTS of the MDS row, left as it is: limbs 0..7 in
//           [0, 3 (2^29 - 1)], |s| < 3.1 p (below).  Round constants and MDS entries are canonical, limbs in [0, 2^29).
//   x = fe29_norm(s + rc)   the one place a carry pass is needed: a limb of s + rc is at most 4 (2^29 - 1) = 2^31 - 4, and
//           fe29_norm's carry is then at most 3, so limb + carry <= 2^31 - 1 never wraps; afterwards the limbs are back in
//           [0, 2^29) (the top limb signed, below 2^26 in magnitude), which fe29_sqr and fe29_mul's narrow side ask for.
//           Without it the S-box input would have limbs of up to 2^31, four times fe29_sqr's bound.
//           Value: |x| < c p with c = 4.1 (a round's input: 3.1 p + p) or c = 5.1 (the first round of a sponge
//           permutation: the normalised state, a message word below p, a round constant below p), so x^2 < 27 p^2,
//           within fe29_sqr's 64 p^2.
//   S-box   x2 = sqr(x) in (-p, c^2 rho p] -- |x2| < p; x4 = sqr(x2) in (-p, rho p]; x5 = mul(x4, x), |x4 x| < c p^2, in
//           (-p - c rho p, c rho p]: |x5| < 1.04 p.  All three results are normalised, so every operand is within the limb
//           bounds and every |a b| is far below 64 p^2.
//   MDS     term = mul(y, m) with m canonical and y either an S-box output (|y| < 1.04 p) or, in a partial round, the
//           normalised x of words 1 and 2 (|y| < c p): |term| < p (1 + c rho) < 1.04 p.  A state word is three of them:
//           |s| < 3.1 p, limbs 0..7 in [0, 3 (2^29 - 1)] -- the fixed point c = 1 + 3 (1 + c / 128) = 4.096 closes the loop.
//   The three terms of an MDS row are three separate products and two additions.  A fused row (one reduction for
//           sum_j m_ij y_j) would put 27 limb products and 9 m p terms of up to 2^58 each into one 64-bit column: 36 2^58
//           exceeds 2^63, so it is not used for any field.
//   out     poseidon_permute ends with fe29_norm of the three words, so that its result can take a message word, go into
//           the LDS of the Merkle tail or through fe29_to_api (limbs below 2^30 in magnitude, |value| < 64 p).
//
// Code size: the rounds are not unrolled.  One full-round body and one partial-round body, each in a loop that is kept as
// a loop (#pragma unroll 1); the two runs of full rounds are the two trips of an outer loop around them.
//
// The product form is a template parameter (h2_field29_chain.hpp's policies).  Measured on the hash kernel (tools/
// poseidon_bench.py): while a SIMD holds one wave or none -- n <= 2^16 lanes on the 256 CUs -- the
// compiler's form is 2-3 % ahead, from two waves per SIMD on the single-chain form is, by 2 % at 2^17 and 5.6 % at 2^20.
// So the hash kernel is instantiated on both and a launch of POSEIDON_CHAIN_MIN_N lanes or more takes the chain form where
// the field has one (Pallas, Vesta); the permutation kernel and the Merkle tail stay on the compiler's form.
#pragma once
#include <hip/hip_runtime.h>

#include "h2_field29.hpp"
#include "h2_field29_chain.hpp"

namespace h2 {

constexpr uint32_t POSEIDON_MAX_ROUNDS = 128;       // r_f + r_p
constexpr uint32_t POSEIDON_THREADS = 256;
constexpr uint32_t POSEIDON_MAX_BLOCKS = 1u << 20;  // beyond that the lanes stride over the rest
constexpr size_t POSEIDON_CHAIN_MIN_N = (1u << 16) + 1;   // more lanes than one wave on every SIMD of the device
// The Merkle walker and update (h2_poseidon_quad.hpp): hashes (paths of a verify call, or hashes of one update level) below
// which a launch takes the QUAD form, four lanes per permutation; from it on the lane form.  The sweep (tools/
// poseidon_merkle_bench.py, verify at depth 20, both forms in one run, best of the windows, ms; DESIGN.md section 7.18 has
// the whole table):
//     n            2^4    2^10   2^12   2^13   2^14   2^15   2^16   2^17    2^18    2^20
//     Pallas lane  6.39   5.61   5.61   5.60   5.69   5.60   5.79   10.72   21.09   83.5
//     Pallas quad  2.69   2.72   2.81   2.94   3.15   5.54   10.01  19.38   38.47   153.6
//     BN254 lane   8.68   7.66   7.67   7.63   7.68   7.62   7.84   14.48   28.26   111.6
//     BN254 quad   3.51   3.53   3.61   3.73   4.17   7.22   13.22  26.03   51.79   207.1
// Up to 2^14 paths -- 2^16 lanes, one wave per SIMD -- the quad form is its own shorter chain (0.40 - 0.55 of the lane
// form); at 2^15 it is two waves per SIMD and level with the lane form (1 - 5 % ahead); at 2^16 the lane form, then one wave
// per SIMD itself, is 1.7 x faster, and 1.8 x where both fill the device.  So: the quad form up to 2^15 hashes, the lane
// form above.  The numbers are those of profiles/poseidon_merkle_times.json.
constexpr size_t POSEIDON_WALK_QUAD_MAX = ((size_t)1 << 15) + 1;
// Merkle tail: levels of at most this many nodes are finished by one workgroup in one launch.  The sweep of tools/
// poseidon_bench.py cannot tell 32 .. 256 apart -- a level is one hash's latency either way -- and
// has 512, where a lane hashes two nodes in turn, behind: the default is the widest level with one node per lane.  The LDS
// of the tail kernel holds up to TAIL_MAX nodes
constexpr uint32_t POSEIDON_MERKLE_TAIL = 256;
constexpr uint32_t POSEIDON_MERKLE_TAIL_MAX = 512;

// entries of the table of (r_f, r_p)
H2_HD constexpr uint32_t poseidon_table_elems(uint32_t r_f, uint32_t r_p) { return (r_f + r_p) * 3 + 9; }

// One constant of the table.  The table is not written while a kernel that reads it runs, and the address is the same in
// every lane: on the device the load goes through the constant address space, which the back end always serves with
// scalar loads (for a plain global pointer it does so only where it can prove that no store of the kernel reaches it)
template <class FS>
H2_HD Fe29<FS> poseidon_const(const Fe29<FS>* p) {
#if defined(__HIP_DEVICE_COMPILE__)
  typedef const __attribute__((address_space(4))) int32_t* ConstPtr;
  const ConstPtr q = (ConstPtr)(const int32_t*)p->v;
  Fe29<FS> r;
#pragma unroll
  for (int i = 0; i < 9; i++) r.v[i] = q[i];
  return r;
#else
  return *p;
#endif
}

template <class FS, class A>
H2_HD Fe29<FS> poseidon_pow5(const Fe29<FS>& x) {
  const Fe29<FS> x2 = A::template sqr<FS>(x);
  const Fe29<FS> x4 = A::template sqr<FS>(x2);
  return A::template mul<FS>(x4, x);
}
// one word of s = M y: three products and two additions, the sum left un-normalised
template <class FS, class A>
H2_HD Fe29<FS> poseidon_mds_row(const Fe29<FS>& y0, const Fe29<FS>& y1, const Fe29<FS>& y2, const Fe29<FS>* row) {
  return fe29_add(fe29_add(A::template mul<FS>(y0, poseidon_const(row)), A::template mul<FS>(y1, poseidon_const(row + 1))),
                  A::template mul<FS>(y2, poseidon_const(row + 2)));
}
// the S-box input (and, in a partial round, words 1 and 2 as they go into the MDS product): s + rc, carries propagated
template <class FS>
H2_HD Fe29<FS> poseidon_add_rc(const Fe29<FS>& s, const Fe29<FS>* rc) {
  return fe29_norm(fe29_add(s, poseidon_const(rc)));
}

// s: three words of magnitude below 3.1 p with limbs 0..7 in [0, 3 (2^29 - 1)] (a canonical or normalised word is one)
// -> the permuted state, normalised, same magnitude.  r_f even, r_f + r_p <= POSEIDON_MAX_ROUNDS
template <class FS, class A = Fe29Compiler>
H2_HD void poseidon_permute(Fe29<FS> s[3], const Fe29<FS>* __restrict__ table, uint32_t r_f, uint32_t r_p) {
  const Fe29<FS>* const mds = table + 3 * (size_t)(r_f + r_p);
  const Fe29<FS>* rc = table;
  const uint32_t half = r_f >> 1;
  Fe29<FS> s0 = s[0], s1 = s[1], s2 = s[2];
#pragma unroll 1
  for (int run = 0; run < 2; run++) {
#pragma unroll 1
    for (uint32_t r = 0; r < half; r++, rc += 3) {
      const Fe29<FS> y0 = poseidon_pow5<FS, A>(poseidon_add_rc(s0, rc + 0));
      const Fe29<FS> y1 = poseidon_pow5<FS, A>(poseidon_add_rc(s1, rc + 1));
      const Fe29<FS> y2 = poseidon_pow5<FS, A>(poseidon_add_rc(s2, rc + 2));
      s0 = poseidon_mds_row<FS, A>(y0, y1, y2, mds);
      s1 = poseidon_mds_row<FS, A>(y0, y1, y2, mds + 3);
      s2 = poseidon_mds_row<FS, A>(y0, y1, y2, mds + 6);
    }
    if (run == 0) {
#pragma unroll 1
      for (uint32_t r = 0; r < r_p; r++, rc += 3) {
        const Fe29<FS> y0 = poseidon_pow5<FS, A>(poseidon_add_rc(s0, rc + 0));
        const Fe29<FS> y1 = poseidon_add_rc(s1, rc + 1);
        const Fe29<FS> y2 = poseidon_add_rc(s2, rc + 2);
        s0 = poseidon_mds_row<FS, A>(y0, y1, y2, mds);
        s1 = poseidon_mds_row<FS, A>(y0, y1, y2, mds + 3);
        s2 = poseidon_mds_row<FS, A>(y0, y1, y2, mds + 6);
      }
    }
  }
  s[0] = fe29_norm(s0);
  s[1] = fe29_norm(s1);
  s[2] = fe29_norm(s2);
}

// ConstantLength<len>: msg = len canonical elements in the API form; cap = len 2^64 in the working form
template <class FS, class A = Fe29Compiler>
H2_HD Fe29<FS> poseidon_hash(const U128* __restrict__ msg, uint32_t len, const Fe29<FS>& cap, const Fe29<FS>* __restrict__ table,
                             uint32_t r_f, uint32_t r_p) {
  Fe29<FS> s[3] = {Fe29<FS>::zero(), Fe29<FS>::zero(), cap};
#pragma unroll 1
  for (uint32_t off = 0; off < len; off += 2) {
    s[0] = fe29_add(s[0], fe29_from_api(fe_load<FS>(msg + 2 * (size_t)off)));
    if (off + 1 < len) s[1] = fe29_add(s[1], fe29_from_api(fe_load<FS>(msg + 2 * (size_t)off + 2)));
    poseidon_permute<FS, A>(s, table, r_f, r_p);
  }
  return s[0];
}
// the same on two words already in the working form (normalised): a Merkle node from its children
template <class FS, class A = Fe29Compiler>
H2_HD Fe29<FS> poseidon_hash2(const Fe29<FS>& a, const Fe29<FS>& b, const Fe29<FS>& cap2, const Fe29<FS>* __restrict__ table,
                              uint32_t r_f, uint32_t r_p) {
  Fe29<FS> s[3] = {a, b, cap2};
  poseidon_permute<FS, A>(s, table, r_f, r_p);
  return s[0];
}

#if defined(__HIPCC__)
// n states of three elements (API form), one lane per state; out may be in itself
template <class FS>
__global__ void __launch_bounds__(POSEIDON_THREADS)
poseidon_permute_kernel(const U128* in, U128* out, size_t n, const Fe29<FS>* __restrict__ table, uint32_t r_f, uint32_t r_p) {
  const size_t stride = (size_t)gridDim.x * POSEIDON_THREADS;
  for (size_t i = (size_t)blockIdx.x * POSEIDON_THREADS + threadIdx.x; i < n; i += stride) {
    Fe29<FS> s[3];
#pragma unroll
    for (int j = 0; j < 3; j++) s[j] = fe29_from_api(fe_load<FS>(in + 6 * i + 2 * j));
    poseidon_permute<FS>(s, table, r_f, r_p);
#pragma unroll
    for (int j = 0; j < 3; j++) fe_store<FS>(out + 6 * i + 2 * j, fe29_to_api(s[j]));
  }
}

// n messages of len elements, msg_stride elements apart -> n elements; one lane per message
template <class FS, class A>
__global__ void __launch_bounds__(POSEIDON_THREADS)
poseidon_hash_kernel(const U128* __restrict__ msgs, uint32_t len, size_t msg_stride, size_t n, U128* __restrict__ out, Fe29<FS> cap,
                     const Fe29<FS>* __restrict__ table, uint32_t r_f, uint32_t r_p) {
  const size_t stride = (size_t)gridDim.x * POSEIDON_THREADS;
  for (size_t i = (size_t)blockIdx.x * POSEIDON_THREADS + threadIdx.x; i < n; i += stride)
    fe_store<FS>(out + 2 * i, fe29_to_api(poseidon_hash<FS, A>(msgs + 2 * i * msg_stride, len, cap, table, r_f, r_p)));
}

// The top of a Merkle tree in ONE workgroup: `width` nodes (a power of two, 1 <= width <= POSEIDON_MERKLE_TAIL_MAX) from
// their 2 width children at `in`, then every level above them up to the root, each level written behind the one before
// at `out` (2 width - 1 nodes in all).  The levels above the first are read from LDS in the working form -- no
// conversion in, no trip through memory -- and a barrier separates a level's writes from the next level's reads; two
// buffers alternate, so a level never overwrites what another lane still reads.  Limb-major layout: lane i's limb l
// at [l][i], no bank conflict on the store and two-way on the stride-two loads.
template <class FS>
__global__ void __launch_bounds__(POSEIDON_THREADS)
poseidon_merkle_tail_kernel(const U128* __restrict__ in, U128* __restrict__ out, uint32_t width, Fe29<FS> cap2,
                            const Fe29<FS>* __restrict__ table, uint32_t r_f, uint32_t r_p) {
  __shared__ int32_t lvl_a[9 * POSEIDON_MERKLE_TAIL_MAX];
  __shared__ int32_t lvl_b[9 * (POSEIDON_MERKLE_TAIL_MAX / 2)];
  const uint32_t t = threadIdx.x;
  int32_t* src = lvl_b;
  int32_t* dst = lvl_a;
  uint32_t src_ld = POSEIDON_MERKLE_TAIL_MAX / 2, dst_ld = POSEIDON_MERKLE_TAIL_MAX;
  bool first = true;
#pragma unroll 1
  for (uint32_t w = width; w >= 1; w >>= 1) {
    for (uint32_t i = t; i < w; i += POSEIDON_THREADS) {
      Fe29<FS> a, b;
      if (first) {
        a = fe29_from_api(fe_load<FS>(in + 4 * (size_t)i));
        b = fe29_from_api(fe_load<FS>(in + 4 * (size_t)i + 2));
      } else {
#pragma unroll
        for (int l = 0; l < 9; l++) {
          a.v[l] = src[l * src_ld + 2 * i];
          b.v[l] = src[l * src_ld + 2 * i + 1];
        }
      }
      const Fe29<FS> h = poseidon_hash2<FS, Fe29Compiler>(a, b, cap2, table, r_f, r_p);
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
#endif  // __HIPCC__

}  // namespace h2
