// h2_poseidon_host.hpp -- the Poseidon parameter generation (host only), one copy for the C ABI (h2_capi.hip:
// h2_poseidon_constants and the kernels' tables) and for the Poseidon circuit (h2_circuits.hpp).
//
// Restates the reference's circuits/src/poseidon/primitives/grain.rs:52-137 (the Grain LFSR), primitives.rs:57-84 (round
// constants by rejection sampling) and mds.rs:5-102 (the Cauchy MDS from the first draw of 2 t distinct values, and its
// inverse in closed form) for t = 3, generic over the field and over (r_f, r_p); num_bits comes from the field: 254 for
// bn256::Fr, 255 for the Pasta fields.  (8, 56) on a Pasta field is the reference's P128Pow5T3, (8, 60) on bn256::Fr is
// poseidon_circuit.rs:19-25's spec.  The judge of all of it is oracle/pyref.py::poseidon_constants.
#pragma once
#include <array>
#include <cstdint>
#include <cstring>
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

// round constants, Cauchy MDS and its inverse over FP for t = 3 (primitives.rs:57-84, mds.rs:5-102)
template <class FP>
Constants<FP> generate(int r_f, int r_p) {
  using F = HF<FP>;
  Constants<FP> k;
  const int t = 3;
  Grain g((int)FP::NUM_BITS, t, r_f, r_p);
  uint8_t b[32];
  for (int r = 0; r < r_f + r_p; r++) {
    std::array<F, 3> row;
    int have = 0;
    while (have < t) {
      g.take(b);
      F v;
      if (F::from_le_bytes_canonical(b, &v)) row[have++] = v;   // rejection sampling: values >= p are skipped
    }
    k.rcs.push_back(row);
  }
  F xs[3], ys[3];
  for (;;) {
    F vals[6];
    for (int i = 0; i < 6; i++) {
      g.take(b);
      vals[i] = F::from_le_bytes_reduce(b);                     // here the bits are reduced, not rejected
    }
    bool distinct = true;
    for (int i = 0; i < 6; i++)
      for (int j = i + 1; j < 6; j++)
        if (vals[i] == vals[j]) distinct = false;
    if (distinct) {
      for (int i = 0; i < 3; i++) { xs[i] = vals[i]; ys[i] = vals[3 + i]; }
      break;
    }
  }
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) k.mds[i][j] = (xs[i] + ys[j]).inv();
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
