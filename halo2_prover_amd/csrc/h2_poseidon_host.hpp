// h2_poseidon_host.hpp -- the Poseidon parameter generation (host only), one copy for the C ABI (h2_capi.hip:
// h2_poseidon_constants and the kernels' tables) and for the Poseidon circuit (h2_circuits.hpp).
//
// Restates the reference's circuits/src/poseidon/primitives/grain.rs:52-137 (the Grain LFSR), primitives.rs:57-84 (round
// constants by rejection sampling) and mds.rs:5-102 (the Cauchy MDS from the first draw of 2 t distinct values, and its
// inverse in closed form -- the inverse for t = 3 only), generic over the field, the width t and (r_f, r_p); num_bits
// comes from the field: 254 for bn256::Fr, 255 for the Pasta fields.  (8, 56) on a Pasta field is the reference's
// P128Pow5T3, (8, 60) on bn256::Fr is poseidon_circuit.rs:19-25's spec.  The judge of all of it is oracle/pyref.py::poseidon_constants.
#pragma once
#include <array>
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>

#include "h2_host.hpp"

namespace h2 {
namespace poseidon {

// -- Grain LFSR of the Poseidon reference parameter generation (poseidon/primitives/grain.rs:52-137)
class Grain {
 public:
  Grain(int num_bits, int t, int r_f, int r_p) : num_bits_(num_bits) {
    const int widths[6] = {2, 4, 12, 12, 10, 10}, values[6] = {1, 0, num_bits, t, r_f, r_p};
    for (int k = 0; k < 6; k++)
      for (int i = 0; i < widths[k]; i++) st_.push_back((values[k] >> (widths[k] - 1 - i)) & 1);
    for (int i = 0; i < 30; i++) st_.push_back(1);
    for (int i = 0; i < 160; i++) raw();
  }
  // num_bits bits, most significant first, as 32 little-endian bytes
  void take(uint8_t out[32]) {
    memset(out, 0, 32);
    for (int i = num_bits_ - 1; i >= 0; i--)
      if (bit()) out[i >> 3] |= (uint8_t)(1u << (i & 7));
  }

 private:
  int raw() {
    const int b = st_[pos_ + 62] ^ st_[pos_ + 51] ^ st_[pos_ + 38] ^ st_[pos_ + 23] ^ st_[pos_ + 13] ^ st_[pos_];
    st_.push_back((uint8_t)b);
    pos_++;
    return b;
  }
  int bit() {
    for (;;) {
      if (raw()) return raw();
      raw();
    }
  }
  std::vector<uint8_t> st_;
  size_t pos_ = 0;
  int num_bits_;
};

template <class FP>
struct Constants {
  std::vector<std::array<HF<FP>, 3>> rcs;     // r_f + r_p rounds
  HF<FP> mds[3][3], minv[3][3];
};
// the same for any width t: rcs[r * t + i], mds[i * t + j]; no inverse (the kernels, h2_poseidon.hpp, need none)
template <class FP>
struct WideConstants {
  int t = 0;
  std::vector<HF<FP>> rcs, mds;
  std::vector<HF<FP>> points;                 // the 2 t Cauchy points the MDS was made of: xs, then ys
};

// round constants and Cauchy MDS over FP for width t (primitives.rs:57-84, mds.rs:5-63: xs = vals[..t], ys = vals[t..])
template <class FP>
WideConstants<FP> generate_wide(int t, int r_f, int r_p) {
  using F = HF<FP>;
  WideConstants<FP> k;
  k.t = t;
  Grain g((int)FP::NUM_BITS, t, r_f, r_p);
  uint8_t b[32];
  while ((int)k.rcs.size() < (r_f + r_p) * t) {
    g.take(b);
    F v;
    if (F::from_le_bytes_canonical(b, &v)) k.rcs.push_back(v);   // rejection sampling: values >= p are skipped
  }
  std::vector<F>& vals = k.points;
  vals.resize(2 * t);
  for (;;) {
    for (int i = 0; i < 2 * t; i++) {
      g.take(b);
      vals[i] = F::from_le_bytes_reduce(b);                      // here the bits are reduced, not rejected
    }
    bool distinct = true;
    for (int i = 0; i < 2 * t; i++)
      for (int j = i + 1; j < 2 * t; j++)
        if (vals[i] == vals[j]) distinct = false;
    if (distinct) break;
  }
  k.mds.resize((size_t)t * t);
  for (int i = 0; i < t; i++)
    for (int j = 0; j < t; j++) k.mds[(size_t)i * t + j] = (vals[i] + vals[t + j]).inv();
  return k;
}

// ---- the sparse form of the partial rounds (h2_poseidon.hpp, widths 5 and 9) ------------------------------------------
// The r_p partial rounds  s <- M sigma(s + c_k)  (sigma: x^5 on word 0 alone) cost t^2 products each.  Split a matrix
//     N = [ n00  v ]  =  S N',     S = [ n00  v Nh^-1 ],   N' = [ 1  0  ]
//         [ w   Nh ]                   [ w    I       ]         [ 0  Nh ]
// N' leaves word 0 alone and is linear on the others, so it commutes with sigma: N sigma(s + c) = S sigma(N' s + N' c).  N' s
// is the output of the round BEFORE, whose matrix thereby becomes N' M, which is split in its turn.  Backwards from the
// last partial round (N_{P-1} = M;  N_k = S_k N'_k;  N_{k-1} = N'_k M) every partial round is left with its sparse S_k
// (a full first row, a full first column, a unit diagonal: 2 t - 1 products) and the full round in front of them takes the
// PRE-MATRIX N'_0 M instead of M.  With y_k = N'_k s_k:  y_{k+1} = S_k sigma(y_k + N'_k c_k),  y_P = s_P.
// The constants: of d_k = N'_k c_k only word 0 passes the S-box, the words 1.. may be added behind it as well, and
// y_k + (0, rest) = S_{k-1} (stuff + q) with q = S_{k-1}^-1 (0, rest): q_0 becomes round k - 1's constant b behind the S-box,
// q_1.. join round k - 1's own rest.  Backwards again, every round keeps two scalars -- a in front of the S-box, b behind
// it -- and the whole vector d0 is added once, in front of partial round 0:
//     round k:   z = (y_0 + a_k)^5 + b_k;   y_0 <- m00 z + sum_j vhat_j y_j;   y_j <- y_j + w_j z   (j >= 1)
// Every S_k is invertible and every Nh is (a product of minors of a Cauchy matrix); an instance for which one is not -- none
// is known -- makes factor_partial_rounds return false.
template <class FP>
struct SparseRounds {
  std::vector<HF<FP>> pre;       // t x t, row-major
  std::vector<HF<FP>> d0;        // t; d0[0] = round 0's a
  std::vector<HF<FP>> rounds;    // r_p x (2 t + 1): a, b, m00, vhat[1 .. t - 1], w[1 .. t - 1]
};
// the inverse of the n x n matrix a (row-major) by Gauss-Jordan elimination; false when it is singular
template <class F>
bool invert_matrix(std::vector<F> a, int n, std::vector<F>* out) {
  std::vector<F> b((size_t)n * n, F::zero());
  for (int i = 0; i < n; i++) b[(size_t)i * n + i] = F::one();
  for (int c = 0; c < n; c++) {
    int piv = c;
    while (piv < n && a[(size_t)piv * n + c].is_zero()) piv++;
    if (piv == n) return false;
    for (int j = 0; j < n; j++) {
      std::swap(a[(size_t)piv * n + j], a[(size_t)c * n + j]);
      std::swap(b[(size_t)piv * n + j], b[(size_t)c * n + j]);
    }
    const F inv = a[(size_t)c * n + c].inv();
    for (int j = 0; j < n; j++) {
      a[(size_t)c * n + j] = a[(size_t)c * n + j] * inv;
      b[(size_t)c * n + j] = b[(size_t)c * n + j] * inv;
    }
    for (int i = 0; i < n; i++) {
      if (i == c || a[(size_t)i * n + c].is_zero()) continue;
      const F f = a[(size_t)i * n + c];
      for (int j = 0; j < n; j++) {
        a[(size_t)i * n + j] = a[(size_t)i * n + j] - f * a[(size_t)c * n + j];
        b[(size_t)i * n + j] = b[(size_t)i * n + j] - f * b[(size_t)c * n + j];
      }
    }
  }
  *out = b;
  return true;
}
template <class FP>
bool factor_partial_rounds(const WideConstants<FP>& k, int r_f, int r_p, SparseRounds<FP>* out) {
  using F = HF<FP>;
  const int t = k.t, u = t - 1, half = r_f / 2;
  SparseRounds<FP> sp;
  sp.d0.assign(t, F::zero());
  sp.rounds.assign((size_t)r_p * (2 * t + 1), F::zero());
  std::vector<F> N = k.mds;                                  // N_k, from the last partial round down
  std::vector<std::vector<F>> d(r_p);                        // d_k = N'_k c_k
  for (int r = r_p - 1; r >= 0; r--) {
    std::vector<F> Nh((size_t)u * u), Nh_inv;
    for (int i = 0; i < u; i++)
      for (int j = 0; j < u; j++) Nh[(size_t)i * u + j] = N[(size_t)(i + 1) * t + j + 1];
    if (!invert_matrix(Nh, u, &Nh_inv)) return false;
    F* e = &sp.rounds[(size_t)r * (2 * t + 1)];
    e[2] = N[0];
    for (int j = 0; j < u; j++) {
      F acc = F::zero();
      for (int i = 0; i < u; i++) acc = acc + N[1 + i] * Nh_inv[(size_t)i * u + j];     // v Nh^-1
      e[3 + j] = acc;
      e[3 + u + j] = N[(size_t)(j + 1) * t];                                             // w
    }
    const F* c = &k.rcs[(size_t)(half + r) * t];
    d[r].assign(t, F::zero());
    d[r][0] = c[0];
    for (int i = 0; i < u; i++)
      for (int j = 0; j < u; j++) d[r][i + 1] = d[r][i + 1] + Nh[(size_t)i * u + j] * c[j + 1];
    std::vector<F> next((size_t)t * t);                      // N'_k M
    for (int j = 0; j < t; j++) next[j] = k.mds[j];
    for (int i = 0; i < u; i++)
      for (int j = 0; j < t; j++) {
        F acc = F::zero();
        for (int m = 0; m < u; m++) acc = acc + Nh[(size_t)i * u + m] * k.mds[(size_t)(m + 1) * t + j];
        next[(size_t)(i + 1) * t + j] = acc;
      }
    N = next;
  }
  sp.pre = N;                                                // r_p = 0: M itself, and nothing else is read
  std::vector<F> carry(u, F::zero());                        // what the rounds behind round r push into its words 1..
  for (int r = r_p - 1; r >= 0; r--) {
    F* e = &sp.rounds[(size_t)r * (2 * t + 1)];
    e[0] = d[r][0];
    std::vector<F> rest(u);
    for (int j = 0; j < u; j++) rest[j] = d[r][j + 1] + carry[j];
    if (r == 0) {
      sp.d0[0] = d[0][0];
      for (int j = 0; j < u; j++) sp.d0[j + 1] = rest[j];
      break;
    }
    // q = S_{r-1}^-1 (0, rest):  q_0 = -(vhat . rest) / (m00 - vhat . w),  q_j = rest_j - w_j q_0
    const F* s = &sp.rounds[(size_t)(r - 1) * (2 * t + 1)];
    F vr = F::zero(), vw = F::zero();
    for (int j = 0; j < u; j++) {
      vr = vr + s[3 + j] * rest[j];
      vw = vw + s[3 + j] * s[3 + u + j];
    }
    const F det = s[2] - vw;
    if (det.is_zero()) return false;
    const F q0 = -(vr * det.inv());
    sp.rounds[(size_t)(r - 1) * (2 * t + 1) + 1] = q0;       // round r - 1's b
    for (int j = 0; j < u; j++) carry[j] = rest[j] - s[3 + u + j] * q0;
  }
  *out = sp;
  return true;
}

// the t = 3 instance with the inverse of its MDS in closed form (mds.rs:64-102): what the Poseidon circuit is built on
template <class FP>
Constants<FP> generate(int r_f, int r_p) {
  using F = HF<FP>;
  Constants<FP> k;
  const WideConstants<FP> w = generate_wide<FP>(3, r_f, r_p);
  for (int r = 0; r < r_f + r_p; r++) k.rcs.push_back({w.rcs[3 * r], w.rcs[3 * r + 1], w.rcs[3 * r + 2]});
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) k.mds[i][j] = w.mds[3 * i + j];
  const F* xs = w.points.data();
  const F* ys = xs + 3;
  auto lag = [](const F* pts, int j, const F& x) {
    F acc = F::one();
    for (int m = 0; m < 3; m++)
      if (m != j) acc = acc * (x - pts[m]) * (pts[j] - pts[m]).inv();
    return acc;
  };
  F nys[3];
  for (int i = 0; i < 3; i++) nys[i] = -ys[i];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) k.minv[i][j] = (xs[j] - nys[i]) * lag(xs, j, nys[i]) * lag(nys, i, xs[j]);
  return k;
}

}  // namespace poseidon
}  // namespace h2
