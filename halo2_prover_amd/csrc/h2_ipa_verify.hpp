// h2_ipa_verify.hpp -- the device side of the IPA batch verifier (h2_ipa_replay_device, h2_ipa_verify_proofs; DESIGN.md
// section 7.17): the Fiat-Shamir replay of `count` proofs, one lane each, and the scalars of one combined check.
//
// Replay.  A proof's transcript is Blake2b over a fixed sequence of pieces: S, then k x (L_j, R_j), then c and f, a challenge
// squeezed after S (twice) and after every R_j.  The sequence is the same for every proof, so a wave walks it in lockstep;
// what differs between lanes is where the caller's prefix left the 128-byte block buffer.  The buffer is a ring of TWO
// blocks per lane in LDS, word w of lane l at ring[w * 64 + l] (a wave's accesses to one word fall on 64 consecutive
// dwords): a piece of up to 66 bytes is written at the lane's own byte offset with constant-indexed register bytes, and
// when it runs past the end of the current block that block is compressed and the other becomes current.  This is Blake2b's
// own rule -- a full block is compressed only once more input follows, the last one is finalised with the flag -- with at
// most one compression per piece, at ONE place in the loop whatever the lanes' offsets are.  Nothing is indexed by a lane
// variable but LDS addresses: the state (16 VGPRs), the message words (32) and the work vector (32) are registers with
// compile-time indices -- the rounds are unrolled by templates, so the message schedule is constants -- and the kernel has
// no scratch.  A squeeze compresses a COPY of the chaining words with the bytes behind `buflen` masked to zero as they are
// read.  64-bit adds and xors are two VALU operations each, the rotations by 32, 24 and 16 move whole bytes and the one by
// 63 is two funnel shifts: all written as plain 64-bit C++, which the back end lowers that way.
//
// Prepare.  One lane per proof turns the replay's row, x3, v and a 128-bit weight w into its rows of the points MSM's scalar
// column, its row of ipa_s_sum_kernel's table (ipa_sum_fill's layout, h2_ipa.hpp) and its three terms w v, w c b_0 z, w f.
// The k inverses 1 / u_j share ONE inversion: the prefix products are parked in the rows the inverses will take.  A zero
// weight -- the proof is not in this check -- writes zero rows and zero terms.  The finish kernel adds the terms in a fixed
// order (one workgroup, a tree in LDS, canonical fe_add: no atomics, the bits do not depend on the grid) and writes
// col[0] -= sum w v and the two tail rows of the table MSM's column.
#pragma once
#include "h2_field.hpp"
#include "h2_field29.hpp"
#include "h2_ipa.hpp"
#include "h2_poly.hpp"

namespace h2 {

constexpr int IPA_REPLAY_THREADS = 64;                    // one wave: the ring's interleave
constexpr uint32_t TRANSCRIPT_STATE_BYTES = 208;          // h2_transcript_state_t: h[8], t, buf[128], buflen, reserved
constexpr int IPA_PREP_THREADS = 64;
constexpr uint32_t IPA_WEIGHT_WORDS = 8;                  // per proof: the weight's 4 words, its row of the sum table, 3 unused

__host__ __device__ constexpr uint32_t blake2b_sigma(int r, int i) {
  constexpr uint8_t S[10][16] = {
      {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}, {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3},
      {11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4}, {7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8},
      {9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13}, {2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9},
      {12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11}, {13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10},
      {6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5}, {10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0}};
  return S[r % 10][i];
}

template <int R, int I>
constexpr uint32_t B2B_S = blake2b_sigma(R, I);          // the message schedule as constants: m[] is never indexed at run time

H2_HD uint64_t blake2b_rotr(uint64_t x, int n) { return (x >> n) | (x << (64 - n)); }

#define H2_B2B_G(a, b, c, d, x, y)                              \
  v[a] = v[a] + v[b] + (x); v[d] = blake2b_rotr(v[d] ^ v[a], 32); \
  v[c] = v[c] + v[d];       v[b] = blake2b_rotr(v[b] ^ v[c], 24); \
  v[a] = v[a] + v[b] + (y); v[d] = blake2b_rotr(v[d] ^ v[a], 16); \
  v[c] = v[c] + v[d];       v[b] = blake2b_rotr(v[b] ^ v[c], 63)

// RFC 7693's F on h with the block m, the byte counter t (below 2^64) and the last-block flag
H2_HD void blake2b_compress(uint64_t (&h)[8], const uint64_t (&m)[16], uint64_t t, bool last) {
  constexpr uint64_t IV[8] = {0x6a09e667f3bcc908ull, 0xbb67ae8584caa73bull, 0x3c6ef372fe94f82bull, 0xa54ff53a5f1d36f1ull,
                              0x510e527fade682d1ull, 0x9b05688c2b3e6c1full, 0x1f83d9abfb41bd6bull, 0x5be0cd19137e2179ull};
  uint64_t v[16];
#pragma unroll
  for (int i = 0; i < 8; i++) {
    v[i] = h[i];
    v[i + 8] = IV[i];
  }
  v[12] ^= t;
  if (last) v[14] = ~v[14];
  ipa_static_for<12>([&](auto R) {
    constexpr int r = decltype(R)::value;
    H2_B2B_G(0, 4, 8, 12, m[(B2B_S<r, 0>)], m[(B2B_S<r, 1>)]);
    H2_B2B_G(1, 5, 9, 13, m[(B2B_S<r, 2>)], m[(B2B_S<r, 3>)]);
    H2_B2B_G(2, 6, 10, 14, m[(B2B_S<r, 4>)], m[(B2B_S<r, 5>)]);
    H2_B2B_G(3, 7, 11, 15, m[(B2B_S<r, 6>)], m[(B2B_S<r, 7>)]);
    H2_B2B_G(0, 5, 10, 15, m[(B2B_S<r, 8>)], m[(B2B_S<r, 9>)]);
    H2_B2B_G(1, 6, 11, 12, m[(B2B_S<r, 10>)], m[(B2B_S<r, 11>)]);
    H2_B2B_G(2, 7, 8, 13, m[(B2B_S<r, 12>)], m[(B2B_S<r, 13>)]);
    H2_B2B_G(3, 4, 9, 14, m[(B2B_S<r, 14>)], m[(B2B_S<r, 15>)]);
  });
#pragma unroll
  for (int i = 0; i < 8; i++) h[i] ^= v[i] ^ v[i + 8];
}
#undef H2_B2B_G

// One lane's transcript (the replay below, the prover's step kernel in h2_ipa_prove.hpp): the chaining words and the byte
// counter in registers, the block buffer the ring of two blocks the header describes, word w at ring[w * STRIDE] -- STRIDE =
// 64 in LDS with `ring` already at the lane's word 0, STRIDE = 1 for a host instantiation
template <int STRIDE>
struct B2bLane {
  uint64_t h[8], t;
  uint32_t buflen, cur;
  uint32_t* ring;

  // byte o (mod 256) of the ring, as an index into its bytes
  H2_HD uint32_t at(uint32_t o) const { return ((o & 255u) >> 2) * (uint32_t)(4 * STRIDE) + (o & 3u); }

  // st: the 52 words of an exported state (a buflen above 128 is read as 128)
  H2_HD void load(const uint32_t* st, uint32_t* ring_) {
    ring = ring_;
#pragma unroll
    for (int i = 0; i < 8; i++) h[i] = (uint64_t)st[2 * i] | ((uint64_t)st[2 * i + 1] << 32);
    t = (uint64_t)st[16] | ((uint64_t)st[17] << 32);
#pragma unroll
    for (int w = 0; w < 32; w++) ring[w * STRIDE] = st[18 + w];
    buflen = st[50] < 128u ? st[50] : 128u;
    cur = 0;
  }
  // the current block's words, the bytes from `valid` on read as zero
  H2_HD void block(uint64_t (&m)[16], uint32_t valid) const {
#pragma unroll
    for (int i = 0; i < 32; i++) {
      const uint32_t w = ring[(cur * 32 + i) * STRIDE];
      const int rem = (int)valid - 4 * i;
      const uint32_t mask = rem >= 4 ? 0xFFFFFFFFu : rem <= 0 ? 0u : (1u << (8 * rem)) - 1u;
      if (i & 1)
        m[i >> 1] |= (uint64_t)(w & mask) << 32;
      else
        m[i >> 1] = w & mask;
    }
  }
  // one piece of up to 66 bytes: the tag, then the first len - 1 bytes of d.  A block that is full with more input behind
  // it is compressed and the other one becomes current: at most one compression per piece
  H2_HD void absorb(const uint32_t (&d)[16], uint32_t tag, uint32_t len) {
    uint8_t* ring8 = (uint8_t*)ring;
    uint32_t pw[17];
    pw[0] = tag | (d[0] << 8);
#pragma unroll
    for (int i = 1; i < 16; i++) pw[i] = (d[i - 1] >> 24) | (d[i] << 8);
    pw[16] = d[15] >> 24;
    const uint32_t base = cur * 128 + buflen;
#pragma unroll
    for (int i = 0; i < 66; i++)
      if ((uint32_t)i < len) ring8[at(base + i)] = (uint8_t)(pw[i >> 2] >> (8 * (i & 3)));
    buflen += len;
    if (buflen > 128) {
      uint64_t m[16];
      block(m, 128);
      t += 128;
      blake2b_compress(h, m, t, false);
      cur ^= 1;
      buflen -= 128;
    }
  }
  // Challenge255: the digest of a COPY of the state, reduced modulo the field, Montgomery limbs
  template <class FS>
  H2_HD Fe<FS> squeeze() const {
    uint64_t m[16], hc[8];
#pragma unroll
    for (int i = 0; i < 8; i++) hc[i] = h[i];
    block(m, buflen);
    blake2b_compress(hc, m, t + buflen, true);
    Fe<FS> lo, hi;
#pragma unroll
    for (int i = 0; i < 4; i++) {
      lo.v[2 * i] = (uint32_t)hc[i];
      lo.v[2 * i + 1] = (uint32_t)(hc[i] >> 32);
      hi.v[2 * i] = (uint32_t)hc[4 + i];
      hi.v[2 * i + 1] = (uint32_t)(hc[4 + i] >> 32);
    }
    return fe_from_wide(lo, hi);
  }
  // the state as it stands, exported: the bytes behind buflen zero
  H2_HD void store(uint32_t* so) const {
    uint64_t m[16];
    block(m, buflen);
#pragma unroll
    for (int i = 0; i < 8; i++) {
      so[2 * i] = (uint32_t)h[i];
      so[2 * i + 1] = (uint32_t)(h[i] >> 32);
    }
    so[16] = (uint32_t)t;
    so[17] = (uint32_t)(t >> 32);
#pragma unroll
    for (int i = 0; i < 16; i++) {
      so[18 + 2 * i] = (uint32_t)m[i];
      so[19 + 2 * i] = (uint32_t)(m[i] >> 32);
    }
    so[50] = buflen;
    so[51] = 0;
  }
};

// Lane p replays proof p (the lanes behind `count` repeat the last proof and store nothing, so the wave stays whole).
// states: count x 208 bytes; points: count x (2k + 1) affine points in the API form with their decompression status;
// scalars: count x 64 bytes, c || f as they stand in the stream; out: count x (k + 4) elements xi, z, u_0 .. u_(k-1), c, f
template <class CV>
__global__ void __launch_bounds__(IPA_REPLAY_THREADS)
ipa_replay_kernel(const uint32_t* __restrict__ states, const U128* __restrict__ points, const uint8_t* __restrict__ point_status,
                  const uint32_t* __restrict__ scalars, U128* __restrict__ out, uint8_t* __restrict__ status,
                  uint32_t* __restrict__ states_out, uint32_t k, uint32_t count) {
  using FS = typename CV::Scalar;
  using FB = typename CV::Base;
  __shared__ uint32_t ring[64 * IPA_REPLAY_THREADS];
  const uint32_t lane = threadIdx.x;
  const uint32_t p_raw = blockIdx.x * IPA_REPLAY_THREADS + lane;
  const bool active = p_raw < count;
  const size_t p = active ? p_raw : count - 1;
  const uint32_t per = 2 * k + 1;
  B2bLane<IPA_REPLAY_THREADS> b;
  b.load(states + p * (TRANSCRIPT_STATE_BYTES / 4), ring + lane);

  uint32_t bad_point = 0, bad_scalar = 0, zero_challenge = 0;
  const uint32_t pieces = 2 * k + 4;
  for (uint32_t piece = 0; piece < pieces; piece++) {
    // piece 0: S; 1: nothing (the second squeeze); 2 + 2j, 3 + 2j: L_j, R_j; 2k + 2, 2k + 3: c, f
    const bool is_scalar = piece >= 2 * k + 2;
    const bool squeeze = !is_scalar && (piece < 2 || (piece & 1));
    uint32_t d[16];
#pragma unroll
    for (int i = 0; i < 16; i++) d[i] = 0;
    uint32_t tag = 0, len = 1;
    if (is_scalar) {
      const uint32_t which = piece - (2 * k + 2);
      Fe<FS> s;
#pragma unroll
      for (int i = 0; i < 8; i++) s.v[i] = d[i] = scalars[p * 16 + which * 8 + i];
      if (!fe_is_canonical(s)) bad_scalar = 1;
      if (active) fe_store<FS>(out + 2 * (p * (k + 4) + k + 2 + which), fe_to_mont(s));
      tag = 2;
      len = 33;
    } else if (piece != 1) {
      const size_t idx = p * per + (piece ? piece - 1 : 0);
      const uint32_t ps = point_status[idx];
      if (ps == 1 || ps == 3) bad_point = 1;
      const Fe<FB> x = fe_from_mont(fe_load<FB>(points + 4 * idx)), y = fe_from_mont(fe_load<FB>(points + 4 * idx + 2));
#pragma unroll
      for (int i = 0; i < 8; i++) {
        d[i] = ps == 2 ? 0u : x.v[i];
        d[8 + i] = ps == 2 ? 0u : y.v[i];
      }
      tag = 1;
      len = squeeze ? 66 : 65;                             // the squeeze's 0x00 rides behind the point
    }
    b.absorb(d, tag, len);
    if (squeeze) {                                         // the digest of a COPY, reduced: Challenge255
      const Fe<FS> ch = b.template squeeze<FS>();
      const uint32_t slot = piece < 2 ? piece : 2 + (piece - 3) / 2;
      if (slot >= 2 && ch.is_zero()) zero_challenge = 1;
      if (active) fe_store<FS>(out + 2 * (p * (k + 4) + slot), ch);
    }
  }
  if (!active) return;
  status[p] = bad_point ? 1 : bad_scalar ? 2 : zero_challenge ? 3 : 0;
  if (states_out) b.store(states_out + p * (TRANSCRIPT_STATE_BYTES / 4));
}

template <class CV>
hipError_t ipa_replay_launch(uint32_t k, size_t count, const void* d_states, const void* d_points, const void* d_point_status,
                             const void* d_scalars, void* d_out, void* d_status, void* d_states_out, hipStream_t s) {
  hipLaunchKernelGGL(ipa_replay_kernel<CV>, dim3((unsigned)((count + IPA_REPLAY_THREADS - 1) / IPA_REPLAY_THREADS)),
                     dim3(IPA_REPLAY_THREADS), 0, s, (const uint32_t*)d_states, (const U128*)d_points, (const uint8_t*)d_point_status,
                     (const uint32_t*)d_scalars, (U128*)d_out, (uint8_t*)d_status, (uint32_t*)d_states_out, k, (uint32_t)count);
  return hipGetLastError();
}

// ---- the scalars of one combined check ----------------------------------------------------------------------------------------
// replay: count x (k + 4) elements (the replay's output); x3, v: count elements; weights: count x IPA_WEIGHT_WORDS words.
// scal: the points MSM's column -- proof p's S, L_0, R_0, ... at rows p (2k + 1) ..., its commitment at row count (2k + 1) + p.
// table: ipa_s_sum_kernel's, row weights[p][4] for a proof in the check.  terms: count x 3 elements
template <class FP>
__global__ void __launch_bounds__(IPA_PREP_THREADS)
ipa_verify_prepare_kernel(const U128* __restrict__ replay, const U128* __restrict__ x3, const U128* __restrict__ v,
                          const uint32_t* __restrict__ weights, U128* scal, int32_t* __restrict__ table, U128* __restrict__ terms,
                          uint32_t k, uint32_t count) {
  using F = Fe<FP>;
  const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= count) return;
  const uint32_t per = 2 * k + 1;
  U128* rows = scal + 2 * p * per;
  U128* own = scal + 2 * ((size_t)count * per + p);
  const uint32_t* wp = weights + p * IPA_WEIGHT_WORDS;
  F w = F::zero();
#pragma unroll
  for (int i = 0; i < 4; i++) w.v[i] = wp[i];
  if (w.is_zero()) {
    const F zero = F::zero();
    for (uint32_t r = 0; r < per; r++) fe_store<FP>(rows + 2 * r, zero);
    fe_store<FP>(own, zero);
#pragma unroll
    for (int i = 0; i < 3; i++) fe_store<FP>(terms + 2 * (3 * p + i), zero);
    return;
  }
  w = fe_to_mont(w);
  const U128* rp = replay + 2 * p * (k + 4);
  const F xi = fe_load<FP>(rp), z = fe_load<FP>(rp + 2), c = fe_load<FP>(rp + 2 * (k + 2)), f = fe_load<FP>(rp + 2 * (k + 3));
  // the prefix products u_0 ... u_(j-1) parked in L_j's row, then one inversion for the k challenges
  F pre = F::one();
  for (uint32_t j = 0; j < k; j++) {
    fe_store<FP>(rows + 2 * (1 + 2 * j), pre);
    pre = fe_mul(pre, fe_load<FP>(rp + 2 * (2 + j)));
  }
  F inv = fe_inv(pre);
  const uint32_t levels = k > IPA_SUM_RUN_LOG ? k : IPA_SUM_RUN_LOG;
  int32_t* trow = table + (size_t)wp[4] * (8 + 9 * levels);
  F b0 = F::one(), cur = fe_load<FP>(x3 + 2 * p);
  for (uint32_t j = k; j-- > 0;) {
    const F u = fe_load<FP>(rp + 2 * (2 + j));
    const F uinv = fe_mul(inv, fe_load<FP>(rows + 2 * (1 + 2 * j)));
    inv = fe_mul(inv, u);
    fe_store<FP>(rows + 2 * (1 + 2 * j), fe_mul(w, uinv));
    fe_store<FP>(rows + 2 * (2 + 2 * j), fe_mul(w, u));
    b0 = fe_mul(b0, fe_add(F::one(), fe_mul(u, cur)));     // compute_b: prod (1 + u_j x3^(2^(k-1-j)))
    cur = fe_sqr(cur);
    const Fe29<FP> op = expr_column_operand(u);            // level k - 1 - j of the sum kernel multiplies by u_j
#pragma unroll
    for (int l = 0; l < 9; l++) trow[8 + 9 * (k - 1 - j) + l] = op.v[l];
  }
  const Fe29<FP> one_op = expr_column_operand(F::one());
  for (uint32_t t = k; t < levels; t++) {
#pragma unroll
    for (int l = 0; l < 9; l++) trow[8 + 9 * t + l] = one_op.v[l];
  }
  fe_store<FP>(rows, fe_mul(w, xi));
  fe_store<FP>(own, w);
  const F wc = fe_mul(w, c), init = fe_neg(wc);
#pragma unroll
  for (int l = 0; l < 8; l++) trow[l] = (int32_t)init.v[l];
  fe_store<FP>(terms + 2 * (3 * p), fe_mul(w, fe_load<FP>(v + 2 * p)));
  fe_store<FP>(terms + 2 * (3 * p + 1), fe_mul(fe_mul(wc, b0), z));
  fe_store<FP>(terms + 2 * (3 * p + 2), fe_mul(w, f));
}

// one workgroup: col[0] -= sum of the terms w v, col[n] = -sum w c b_0 z, col[n + 1] = -sum w f
template <class FP>
__global__ void __launch_bounds__(IPA_THREADS)
ipa_verify_finish_kernel(const U128* __restrict__ terms, uint32_t count, U128* __restrict__ col, size_t n) {
  using F = Fe<FP>;
  __shared__ uint32_t lds[3][8][IPA_THREADS];              // [sum][limb][thread]
  const uint32_t t = threadIdx.x;
  F acc[3] = {F::zero(), F::zero(), F::zero()};
  for (uint32_t p = t; p < count; p += IPA_THREADS) {
#pragma unroll
    for (int c = 0; c < 3; c++) acc[c] = fe_add(acc[c], fe_load<FP>(terms + 2 * ((size_t)3 * p + c)));
  }
  for (uint32_t st = IPA_THREADS / 2; st >= 1; st >>= 1) {
#pragma unroll
    for (int c = 0; c < 3; c++)
#pragma unroll
      for (int l = 0; l < 8; l++) lds[c][l][t] = acc[c].v[l];
    __syncthreads();
    if (t < st) {
#pragma unroll
      for (int c = 0; c < 3; c++) {
        F o;
#pragma unroll
        for (int l = 0; l < 8; l++) o.v[l] = lds[c][l][t + st];
        acc[c] = fe_add(acc[c], o);
      }
    }
    __syncthreads();
  }
  if (t == 0) {
    fe_store<FP>(col, fe_sub(fe_load<FP>(col), acc[0]));
    fe_store<FP>(col + 2 * n, fe_neg(acc[1]));
    fe_store<FP>(col + 2 * (n + 1), fe_neg(acc[2]));
  }
}

template <class FP>
hipError_t ipa_verify_prepare_launch(const void* d_replay, const void* d_x3, const void* d_v, const void* d_weights, void* d_scal,
                                     void* d_table, void* d_terms, uint32_t k, size_t count, hipStream_t s) {
  hipLaunchKernelGGL(ipa_verify_prepare_kernel<FP>, dim3((unsigned)((count + IPA_PREP_THREADS - 1) / IPA_PREP_THREADS)),
                     dim3(IPA_PREP_THREADS), 0, s, (const U128*)d_replay, (const U128*)d_x3, (const U128*)d_v,
                     (const uint32_t*)d_weights, (U128*)d_scal, (int32_t*)d_table, (U128*)d_terms, k, (uint32_t)count);
  return hipGetLastError();
}

template <class FP>
hipError_t ipa_verify_finish_launch(const void* d_terms, size_t count, void* d_col, uint32_t k, hipStream_t s) {
  hipLaunchKernelGGL(ipa_verify_finish_kernel<FP>, dim3(1), dim3(IPA_THREADS), 0, s, (const U128*)d_terms, (uint32_t)count,
                     (U128*)d_col, (size_t)1 << k);
  return hipGetLastError();
}

}  // namespace h2
