// h2_ipa_prove.hpp -- the device side of the IPA prover's transcript (h2_ipa_prove_rounds_device, h2_ipa_create_proofs;
// DESIGN.md section 7.20): between two rounds of m openings in lockstep nothing goes through the host.
//
// The step kernel.  One lane per opening (m <= IPA_MAX_BATCH = 64: one wave), launched behind every round's MSM and once
// behind the final kernel.  Behind round j lane i takes L_j || R_j as the MSM's affine finish leaves them, writes their
// wire form into the opening's proof, absorbs them, squeezes u_j, inverts it, adds l_j / u_j + r_j u_j to f_i and writes the
// rows of the state's scalar table (IpaBatchLayout::scal) that the next round's kernels read: u_j, 1 / u_j, and the next
// round's blinds out of the array of all blinds the call uploaded once (row 2, z, stands from that upload on).  Behind
// the final kernel it writes c and f behind the points, absorbs them and stores the midstate.  The Blake2b state of a lane
// lives in the prove state between the launches in its exported form (h2_transcript_state_t), so a launch starts as
// ipa_replay_kernel does and ends as it ends.
//
// The transcript of a lane is B2bLane: ipa_replay_kernel's ring of two blocks (h2_ipa_verify.hpp), word w of the lane at
// ring[w * STRIDE] -- STRIDE = 64 in LDS, one lane's words 64 dwords apart, and STRIDE = 1 for the host instantiation the
// CPU tests run (h2_selftest_ipa_step).
//
// The inversion sits on the critical path of every round, in a lone wave, so it is not fe_inv's Fermat chain (about 380
// dependent products) but Bernstein and Yang's divsteps ("Fast constant-time gcd computation and modular inversion", 2019)
// in the half-delta form, in batches of 30 on the low words: a batch is 30 steps on two 32-bit words that build a 2 x 2
// matrix of 31-bit entries, then that matrix applied to f, g (exactly: the low 30 bits cancel) and to d, e modulo p.  The
// number of steps is FIXED, 20 batches = 600 >= the 590 that bring any g below a modulus of up to 256 bits to zero, so the
// control flow is the same in every lane and for every input; the result is the canonical inverse, and 0 |-> 0 (g = 0
// never changes f = p nor d = 0).
#pragma once
#include "h2_field.hpp"
#include "h2_ipa.hpp"
#include "h2_ipa_verify.hpp"
#include "h2_poly.hpp"

namespace h2 {

// ---- 1 / a by a fixed number of divsteps ------------------------------------------------------------------------------------
namespace inv30 {
constexpr int32_t M30 = (1 << 30) - 1;
constexpr int BATCHES = 20;                              // x 30 steps

// bits [30 i, 30 i + 30) of the modulus
template <class FP>
H2_HD constexpr int32_t modulus(int i) {
  const int word = (30 * i) >> 5, sh = (30 * i) & 31;
  const uint64_t w = (uint64_t)FP::P(word) | (word + 1 < 8 ? (uint64_t)FP::P(word + 1) << 32 : 0);
  return (int32_t)((w >> sh) & (uint64_t)M30);
}

struct Mat {
  int32_t u, v, q, r;
};

// 30 divsteps on the low words: (f, g) -> (u f + v g, q f + r g) / 2^30.  zeta = -(delta + 1/2)
H2_HD int32_t divsteps(int32_t zeta, uint32_t f, uint32_t g, Mat& t) {
  uint32_t u = 1, v = 0, q = 0, r = 1;
#pragma unroll
  for (int i = 0; i < 30; i++) {
    uint32_t c1 = (uint32_t)(zeta >> 31);                // delta > 0
    const uint32_t c2 = 0u - (g & 1u);                   // g odd
    const uint32_t x = (f ^ c1) - c1, y = (u ^ c1) - c1, z = (v ^ c1) - c1;
    g += x & c2;
    q += y & c2;
    r += z & c2;
    c1 &= c2;                                            // both: (f, g) <- (g, (g - f) / 2), delta <- 1 - delta
    zeta = (int32_t)((uint32_t)zeta ^ c1) - 1;
    f += g & c1;
    u += q & c1;
    v += r & c1;
    g >>= 1;
    u <<= 1;
    v <<= 1;
  }
  t.u = (int32_t)u;
  t.v = (int32_t)v;
  t.q = (int32_t)q;
  t.r = (int32_t)r;
  return zeta;
}

// (f, g) <- t (f, g) / 2^30, exact
H2_HD void update_fg(int32_t (&f)[9], int32_t (&g)[9], const Mat& t) {
  int64_t cf = (int64_t)t.u * f[0] + (int64_t)t.v * g[0];
  int64_t cg = (int64_t)t.q * f[0] + (int64_t)t.r * g[0];
  cf >>= 30;
  cg >>= 30;
#pragma unroll
  for (int i = 1; i < 9; i++) {
    cf += (int64_t)t.u * f[i] + (int64_t)t.v * g[i];
    cg += (int64_t)t.q * f[i] + (int64_t)t.r * g[i];
    f[i - 1] = (int32_t)cf & M30;
    g[i - 1] = (int32_t)cg & M30;
    cf >>= 30;
    cg >>= 30;
  }
  f[8] = (int32_t)cf;
  g[8] = (int32_t)cg;
}

// (d, e) <- t (d, e) / 2^30 modulo p, both kept in (-2p, p): a multiple of p makes the low 30 bits vanish
template <class FP>
H2_HD void update_de(int32_t (&d)[9], int32_t (&e)[9], const Mat& t) {
  constexpr uint32_t PINV = (0u - FP::INV) & (uint32_t)M30;      // p^-1 mod 2^30
  const int32_t sd = d[8] >> 31, se = e[8] >> 31;
  int32_t md = (t.u & sd) + (t.v & se), me = (t.q & sd) + (t.r & se);
  int64_t cd = (int64_t)t.u * d[0] + (int64_t)t.v * e[0];
  int64_t ce = (int64_t)t.q * d[0] + (int64_t)t.r * e[0];
  md -= (int32_t)((PINV * (uint32_t)cd + (uint32_t)md) & (uint32_t)M30);
  me -= (int32_t)((PINV * (uint32_t)ce + (uint32_t)me) & (uint32_t)M30);
  cd += (int64_t)modulus<FP>(0) * md;
  ce += (int64_t)modulus<FP>(0) * me;
  cd >>= 30;
  ce >>= 30;
#pragma unroll
  for (int i = 1; i < 9; i++) {
    cd += (int64_t)t.u * d[i] + (int64_t)t.v * e[i] + (int64_t)modulus<FP>(i) * md;
    ce += (int64_t)t.q * d[i] + (int64_t)t.r * e[i] + (int64_t)modulus<FP>(i) * me;
    d[i - 1] = (int32_t)cd & M30;
    e[i - 1] = (int32_t)ce & M30;
    cd >>= 30;
    ce >>= 30;
  }
  d[8] = (int32_t)cd;
  e[8] = (int32_t)ce;
}
}  // namespace inv30

// the canonical inverse of a canonical a as PLAIN integers (no Montgomery factor on either side); 0 -> 0
template <class FP>
H2_HD Fe<FP> fe_inv_divsteps_plain(const Fe<FP>& a) {
  using namespace inv30;
  int32_t d[9], e[9], f[9], g[9];
#pragma unroll
  for (int i = 0; i < 9; i++) {
    const int word = (30 * i) >> 5, sh = (30 * i) & 31;
    const uint64_t w = (uint64_t)a.v[word] | (word + 1 < 8 ? (uint64_t)a.v[word + 1] << 32 : 0);
    g[i] = (int32_t)((w >> sh) & (uint64_t)M30);
    f[i] = modulus<FP>(i);
    d[i] = 0;
    e[i] = i == 0 ? 1 : 0;
  }
  int32_t zeta = -1;                                     // delta = 1/2
  for (int b = 0; b < BATCHES; b++) {
    Mat t;
    zeta = divsteps(zeta, (uint32_t)f[0], (uint32_t)g[0], t);
    update_de<FP>(d, e, t);
    update_fg(f, g, t);
  }
  // g = 0 and f = +-1 (f = p for a = 0): the inverse is d times the sign of f, brought from (-2p, p) to [0, p)
  auto carry = [&]() {
#pragma unroll
    for (int i = 0; i < 8; i++) {
      d[i + 1] += d[i] >> 30;
      d[i] &= M30;
    }
  };
  int32_t add = d[8] >> 31;
  const int32_t neg = f[8] >> 31;
#pragma unroll
  for (int i = 0; i < 9; i++) {
    d[i] += modulus<FP>(i) & add;
    d[i] = (d[i] ^ neg) - neg;
  }
  carry();
  add = d[8] >> 31;
#pragma unroll
  for (int i = 0; i < 9; i++) d[i] += modulus<FP>(i) & add;
  carry();
  Fe<FP> r;
#pragma unroll
  for (int w = 0; w < 8; w++) {
    const int i = (32 * w) / 30, sh = (32 * w) % 30;
    uint64_t x = (uint64_t)(uint32_t)d[i] >> sh | (uint64_t)(uint32_t)d[i + 1] << (30 - sh);
    if (i + 2 < 9) x |= (uint64_t)(uint32_t)d[i + 2] << (60 - sh);
    r.v[w] = (uint32_t)x;
  }
  return r;
}

// fe_inv on Montgomery limbs: the stored a R gives a^-1 R^-1, two products with R^2 make it a^-1 R
template <class FP>
H2_HD Fe<FP> fe_inv_divsteps(const Fe<FP>& a) {
  return fe_to_mont(fe_to_mont(fe_inv_divsteps_plain(a)));
}

// ---- one lane's byte work (on B2bLane, h2_ipa_verify.hpp) -----------------------------------------------------------------------
// The byte work behind a round: lr = L || R, affine, Montgomery limbs of the base field, the identity (0, 0) -- whose
// coordinates are zero in either form, so it needs no case of its own: 64 zero bytes absorbed, 32 zero bytes on the wire.
// wire: the 16 words of the two Pasta wire forms (x little-endian, bit 255 the parity of y).  Returns u (Montgomery limbs)
template <class CV, int STRIDE>
H2_HD Fe<typename CV::Scalar> ipa_step_points(B2bLane<STRIDE>& b, const Fe<typename CV::Base> (&lr)[4], uint32_t (&wire)[16]) {
  using FB = typename CV::Base;
#pragma unroll
  for (int pt = 0; pt < 2; pt++) {
    const Fe<FB> x = fe_from_mont(lr[2 * pt]), y = fe_from_mont(lr[2 * pt + 1]);
    uint32_t d[16];
#pragma unroll
    for (int i = 0; i < 8; i++) {
      d[i] = wire[8 * pt + i] = x.v[i];
      d[8 + i] = y.v[i];
    }
    wire[8 * pt + 7] |= (y.v[0] & 1u) << 31;
    b.absorb(d, 1, pt ? 66 : 65);                        // the squeeze's 0x00 rides behind R
  }
  return b.template squeeze<typename CV::Scalar>();
}

// common_scalar of a scalar given as Montgomery limbs; canon: its 8 canonical words, as they go to the proof
template <class FS, int STRIDE>
H2_HD void ipa_step_scalar(B2bLane<STRIDE>& b, const Fe<FS>& s, uint32_t (&canon)[8]) {
  const Fe<FS> c = fe_from_mont(s);
  uint32_t d[16];
#pragma unroll
  for (int i = 0; i < 8; i++) {
    d[i] = canon[i] = c.v[i];
    d[8 + i] = 0;
  }
  b.absorb(d, 2, 33);
}

// What a lane does with its challenge: uinv = 1 / u (INV 0: by divsteps, 1: fe_inv's Fermat chain, the comparison),
// f += l / u + r u.  Returns 1 for u = 0, whose "inverse" is 0 by either form: no division, no trap, and the caller flags
// the opening
template <class FS, int INV>
H2_HD uint32_t ipa_step_fold(const Fe<FS>& u, const Fe<FS>& l, const Fe<FS>& r, Fe<FS>& f, Fe<FS>& uinv) {
  if constexpr (INV == 0)
    uinv = fe_inv_divsteps(u);
  else
    uinv = fe_inv(u);
  f = fe_add(f, fe_add(fe_mul(l, uinv), fe_mul(r, u)));
  return u.is_zero() ? 1u : 0u;
}

// ---- the prove state ---------------------------------------------------------------------------------------------------------
// What h2_ipa_prove_rounds_device keeps behind IpaBatchLayout, in bytes from the start of the state: all blinds (opening i:
// l_0, r_0, l_1, r_1, ...), f, the midstates, and the buffer the rounds' MSMs (m x L || R, affine) and the final kernel
// (m x c || b_0) write.  The scalar table is the end of IpaBatchLayout, so the table, the blinds, f and the midstates are
// ONE range: the call's single upload
struct IpaProveLayout {
  size_t blinds, f, states, lr, total;
  IpaProveLayout(uint32_t k, size_t m) {
    blinds = IpaBatchLayout(k, m).total * 32;
    f = blinds + m * 2 * k * 32;
    states = f + m * 32;
    lr = states + m * TRANSCRIPT_STATE_BYTES;
    total = lr + m * 128;
  }
};

constexpr int IPA_STEP_THREADS = 64;                      // one wave: the ring's interleave
static_assert(IPA_MAX_BATCH <= IPA_STEP_THREADS, "a lane per opening in one wave");

// j < k: behind round j; j == k: behind the final kernel.  INV: 0 divsteps, 1 fe_inv's Fermat chain (for the comparison).
// tail: m x (2k + 2) x 32 bytes; states_out: null or m x 208 bytes; status: m words, written behind round 0
template <class CV, int INV>
__global__ void __launch_bounds__(IPA_STEP_THREADS)
ipa_prove_step_kernel(U128* st, IpaBatchLayout L, IpaProveLayout P, uint32_t k, uint32_t j, uint32_t* __restrict__ tail,
                      uint32_t* __restrict__ states_out, uint32_t* __restrict__ status) {
  using FS = typename CV::Scalar;
  using FB = typename CV::Base;
  __shared__ uint32_t ring[64 * IPA_STEP_THREADS];
  const uint32_t lane = threadIdx.x;
  const bool active = lane < L.m;                        // the lanes behind m repeat the last opening and store nothing
  const size_t o = active ? lane : L.m - 1;
  char* base = (char*)st;
  uint32_t* state = (uint32_t*)(base + P.states) + o * (TRANSCRIPT_STATE_BYTES / 4);
  uint32_t* proof = tail + o * (2 * (size_t)k + 2) * 8;
  B2bLane<IPA_STEP_THREADS> b;
  b.load(state, ring + lane);
  const U128* lr = (const U128*)(base + P.lr);
  U128* fp = (U128*)(base + P.f) + 2 * o;
  if (j < k) {
    Fe<FB> pts[4];
#pragma unroll
    for (int i = 0; i < 4; i++) pts[i] = fe_load<FB>(lr + 8 * o + 2 * i);
    uint32_t wire[16];
    const Fe<FS> u = ipa_step_points<CV, IPA_STEP_THREADS>(b, pts, wire);
    const U128* blinds = (const U128*)(base + P.blinds) + 2 * (o * 2 * k);
    Fe<FS> uinv, f = fe_load<FS>(fp);
    const uint32_t zero = ipa_step_fold<FS, INV>(u, fe_load<FS>(blinds + 2 * (2 * j)), fe_load<FS>(blinds + 2 * (2 * j + 1)), f, uinv);
    if (active) {
#pragma unroll
      for (int i = 0; i < 16; i++) proof[16 * j + i] = wire[i];
      fe_store<FS>(fp, f);
      U128* table = st + 2 * L.scal;
      fe_store<FS>(table + 2 * o, u);
      fe_store<FS>(table + 2 * (L.m + o), uinv);
      if (j + 1 < k) {
        fe_store<FS>(table + 2 * (3 * L.m + o), fe_load<FS>(blinds + 2 * (2 * j + 2)));
        fe_store<FS>(table + 2 * (4 * L.m + o), fe_load<FS>(blinds + 2 * (2 * j + 3)));
      }
      if (j == 0)                                        // a zero challenge: the opening's proof is void
        status[o] = zero;
      else if (zero)
        status[o] = 1u;
      b.store(state);
    }
  } else {
    const Fe<FS> c = fe_load<FS>(lr + 4 * o), f = fe_load<FS>(fp);
    uint32_t cw[8], fw[8];
    ipa_step_scalar<FS, IPA_STEP_THREADS>(b, c, cw);
    ipa_step_scalar<FS, IPA_STEP_THREADS>(b, f, fw);
    if (active) {
#pragma unroll
      for (int i = 0; i < 8; i++) {
        proof[16 * k + i] = cw[i];
        proof[16 * k + 8 + i] = fw[i];
      }
      b.store(state);
      if (states_out) b.store(states_out + o * (TRANSCRIPT_STATE_BYTES / 4));
    }
  }
}

template <class CV>
hipError_t ipa_prove_step_launch(uint32_t k, uint32_t j, size_t m, void* d_state, void* d_tail, void* d_states_out, void* d_status,
                                 int inv_form, hipStream_t s) {
  const IpaBatchLayout L(k, m);
  const IpaProveLayout P(k, m);
  if (inv_form == 1)
    hipLaunchKernelGGL((ipa_prove_step_kernel<CV, 1>), dim3(1), dim3(IPA_STEP_THREADS), 0, s, (U128*)d_state, L, P, k, j, (uint32_t*)d_tail,
                       (uint32_t*)d_states_out, (uint32_t*)d_status);
  else
    hipLaunchKernelGGL((ipa_prove_step_kernel<CV, 0>), dim3(1), dim3(IPA_STEP_THREADS), 0, s, (U128*)d_state, L, P, k, j, (uint32_t*)d_tail,
                       (uint32_t*)d_states_out, (uint32_t*)d_status);
  return hipGetLastError();
}

}  // namespace h2
