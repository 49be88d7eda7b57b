// h2_opening.hpp -- what is evaluated and opened where: the opening plan of a key, and the pieces of the two multi-open
// schemes that prover and verifier share (SHPLONK's rotation sets, interpolation).
#pragma once
#include <set>

#include "h2_circuits.hpp"
#include "h2_product_dev.hpp"

namespace h2 {
namespace product {

// ---- the opening plan: which polynomial is evaluated and opened at which rotation of x, in which order ----------------------
// A property of the circuit, its permutation sets and the blinding factor, so of the key: built once at keygen and read
// by create_proof, replay_proof and the batch verifier (and dumped by h2_selftest_host what = 9).
enum PolyKind { POLY_ADVICE = 0, POLY_FIXED, POLY_SIGMA, POLY_Z, POLY_RANDOM, POLY_H };
struct Opening {
  int kind, index;       // the polynomial: a PolyKind and the column, the permutation column or the set (0 for random, h)
  int rot;               // rows: the point is x w^rot
  int eval;              // index of its value in `evals`; -1 for h, whose value the transcript does not carry
};
struct OpeningPlan {
  bool shplonk = false;
  std::vector<Opening> evals;      // in the order the evaluations go onto the transcript
  std::vector<Opening> queries;    // in the multi-open's batching order
  // where the groups of `evals` start (advice at 0); set i's z@0, z@1[, z@-(bf+1)] from z0 + 3 i
  size_t fixed0 = 0, random_at = 0, sigma0 = 0, z0 = 0;
  // commitments in front of the evaluations (advice, permutation products, the random polynomial, the quotient pieces)
  // and opening points behind them: one per distinct rotation for GWC, h1 and h2 for SHPLONK
  uint32_t leading = 0, opening_points = 0;
  // Where the compressed points of a proof sit, ascending: fixed by the circuit, not by the challenges.  Should a replay
  // read a point anywhere else it takes the square root itself (Transcript::read_point): a miscount costs time, never a
  // decision (h2_verify_proofs decompresses the points at these offsets ahead of the replays)
  std::vector<uint32_t> point_offsets;
  // what = 9's record (include/h2hip_selftest.h)
  std::vector<uint8_t> dump() const {
    std::vector<int32_t> w = {shplonk, (int32_t)leading, (int32_t)evals.size(), (int32_t)opening_points, (int32_t)queries.size()};
    w.insert(w.end(), point_offsets.begin(), point_offsets.end());
    for (auto& e : evals) w.insert(w.end(), {e.kind, e.index, e.rot});
    for (auto& q : queries) w.insert(w.end(), {q.kind, q.index, q.rot, q.eval});
    return std::vector<uint8_t>((const uint8_t*)w.data(), (const uint8_t*)(w.data() + w.size()));
  }
};
// `sets`: the permutation columns of each grand product (key_shape); n = 2^k rows
inline OpeningPlan opening_plan(const Circuit& C, const std::vector<std::vector<int>>& sets, int bf, uint32_t k, bool shplonk) {
  OpeningPlan L;
  L.shplonk = shplonk;
  const int ns = (int)sets.size(), np = (int)C.permutation_columns.size();
  auto eval = [&](int kind, int index, int rot) { L.evals.push_back({kind, index, rot, (int)L.evals.size()}); };
  for (auto& q : C.advice_queries) eval(POLY_ADVICE, q.first, q.second);
  L.fixed0 = L.evals.size();
  for (auto& q : C.fixed_queries) eval(POLY_FIXED, q.first, q.second);
  L.random_at = L.evals.size();
  eval(POLY_RANDOM, 0, 0);
  L.sigma0 = L.evals.size();
  for (int j = 0; j < np; j++) eval(POLY_SIGMA, j, 0);
  L.z0 = L.evals.size();
  for (int i = 0; i < ns; i++) {
    eval(POLY_Z, i, 0);
    eval(POLY_Z, i, 1);
    if (i + 1 < ns) eval(POLY_Z, i, -(bf + 1));
  }
  auto ask = [&](size_t at) { L.queries.push_back(L.evals[at]); };
  for (size_t qi = 0; qi < L.fixed0; qi++) ask(qi);
  for (int i = 0; i < ns; i++) {
    ask(L.z0 + 3 * i);
    ask(L.z0 + 3 * i + 1);
  }
  for (int i = ns - 1; i-- > 0;) ask(L.z0 + 3 * i + 2);
  for (size_t qi = L.fixed0; qi < L.random_at; qi++) ask(qi);
  for (int j = 0; j < np; j++) ask(L.sigma0 + j);
  L.queries.push_back({POLY_H, 0, 0, -1});
  ask(L.random_at);
  // GWC's distinct points x w^rot: the distinct rotations mod n, for any x != 0
  const int64_t n = (int64_t)1 << k;
  std::set<int64_t> rots;
  for (auto& q : L.queries) rots.insert(((q.rot % n) + n) % n);
  L.opening_points = shplonk ? 2 : (uint32_t)rots.size();
  L.leading = (uint32_t)(C.num_advice + ns + 1 + (C.degree - 1));
  for (uint32_t i = 0; i < L.leading; i++) L.point_offsets.push_back(32 * i);
  for (uint32_t i = 0; i < L.opening_points; i++) L.point_offsets.push_back(32 * (L.leading + (uint32_t)L.evals.size() + i));
  return L;
}

// coefficients of the polynomial of degree < |points| through (points[i], values[i])
inline std::vector<Fr> interpolate(const std::vector<Fr>& points, const std::vector<Fr>& values) {
  std::vector<Fr> out(points.size(), Fr::zero());
  for (size_t i = 0; i < points.size(); i++) {
    std::vector<Fr> term(1, Fr::one());
    Fr den = Fr::one();
    for (size_t j = 0; j < points.size(); j++) {
      if (j == i) continue;
      std::vector<Fr> nt(term.size() + 1, Fr::zero());
      for (size_t dg = 0; dg < term.size(); dg++) {
        nt[dg] -= term[dg] * points[j];
        nt[dg + 1] += term[dg];
      }
      term = nt;
      den *= points[i] - points[j];
    }
    const Fr scale = values[i] * den.inv();
    for (size_t dg = 0; dg < term.size(); dg++) out[dg] += term[dg] * scale;
  }
  return out;
}
inline Fr horner(const std::vector<Fr>& c, const Fr& x) {
  Fr acc = Fr::zero();
  for (size_t i = c.size(); i-- > 0;) acc = acc * x + c[i];
  return acc;
}

// the rotation sets of SHPLONK: polynomials in first-appearance order with their (sorted) point sets, grouped by set
struct ShplonkSets {
  struct Member {
    Col poly;
    std::map<std::array<uint8_t, 32>, Fr> evals;    // by point
    int commitment = -1;                             // verifier side: index into its commitment list
  };
  struct Group {
    std::vector<Fr> points;                          // sorted
    std::vector<Member> members;
  };
  std::vector<Group> groups;
  std::vector<Fr> super;                             // sorted union
};
inline std::array<uint8_t, 32> fr_key(const Fr& f) {
  std::array<uint8_t, 32> b;
  memcpy(b.data(), f.v.v, 32);
  return b;
}
// `ids[i]` identifies the polynomial of query i (prover: its device pointer; verifier: a commitment index)
inline ShplonkSets shplonk_sets(const std::vector<Fr>& pts, const std::vector<Fr>& evs, const std::vector<uintptr_t>& ids) {
  struct Poly {
    uintptr_t id;
    std::vector<Fr> points;
    std::map<std::array<uint8_t, 32>, Fr> evals;
  };
  std::vector<Poly> polys;
  for (size_t i = 0; i < pts.size(); i++) {
    Poly* p = nullptr;
    for (auto& q : polys)
      if (q.id == ids[i]) p = &q;
    if (!p) {
      polys.push_back({ids[i], {}, {}});
      p = &polys.back();
    }
    if (std::find(p->points.begin(), p->points.end(), pts[i]) == p->points.end()) {
      p->points.push_back(pts[i]);
      p->evals[fr_key(pts[i])] = evs[i];
    }
  }
  ShplonkSets S;
  std::set<std::array<uint8_t, 32>> seen;
  for (auto& p : polys) {
    std::vector<Fr> pset = p.points;
    std::sort(pset.begin(), pset.end());
    ShplonkSets::Group* g = nullptr;
    for (auto& gg : S.groups)
      if (gg.points == pset) g = &gg;
    if (!g) {
      S.groups.push_back({pset, {}});
      g = &S.groups.back();
    }
    ShplonkSets::Member m;
    m.poly = (Col)p.id;
    m.commitment = (int)p.id;
    m.evals = p.evals;
    g->members.push_back(m);
    for (auto& pt : pset)
      if (seen.insert(fr_key(pt)).second) S.super.push_back(pt);
  }
  std::sort(S.super.begin(), S.super.end());
  return S;
}

}  // namespace product
}  // namespace h2
