// h2_verify.hpp -- verify_proof and the batch verifier: the transcript's replay, the two combinations behind the
// pairing check, and many proofs of one circuit behind one check.
#pragma once
#include "h2_keygen.hpp"

namespace h2 {
namespace product {

// ---- verify_proof --------------------------------------------------------------------------------------------------------------
// `tag` names the point within one proof's replay (the same point always under the same tag): the batch verifier adds up
// scalars by tag instead of comparing points
struct MsmTerm {
  Fr first;
  G1 second;
  int tag;
};
struct MsmTerms {
  std::vector<MsmTerm> t;
  void append(const Fr& s, const G1& p, int tag = -1) { t.push_back({s, p, tag}); }
  void scale(const Fr& f) {
    for (auto& x : t) x.first *= f;
  }
  void add(const MsmTerms& o) { t.insert(t.end(), o.t.begin(), o.t.end()); }
};

// the group elements of up to four MsmTerms, on the GPU side by side: equal points merged, the rest through msm_small_run
inline std::vector<G1> msm_eval(Dev& d, const std::vector<const MsmTerms*>& jobs) {
  const size_t count = jobs.size();
  std::vector<std::vector<uint8_t>> pts(count), sc(count);
  for (size_t j = 0; j < count; j++) {
    std::vector<std::pair<G1, Fr>> merged;
    for (auto& st : jobs[j]->t) {
      if (st.second.inf || st.first.is_zero()) continue;
      bool found = false;
      for (auto& mg : merged)
        if (mg.first == st.second) {
          mg.second += st.first;
          found = true;
        }
      if (!found) merged.push_back({st.second, st.first});
    }
    const size_t m = merged.size();
    pts[j].resize(m * 64);
    sc[j].resize(m * 32);
    for (size_t i = 0; i < m; i++) {
      memcpy(pts[j].data() + 64 * i, merged[i].first.x.v.v, 32);
      memcpy(pts[j].data() + 64 * i + 32, merged[i].first.y.v.v, 32);
      memcpy(sc[j].data() + 32 * i, merged[i].second.v.v, 32);
    }
  }
  return msm_small_run(d, pts, sc);
}

// verify_proof in two halves.  replay_proof hashes the transcript and arrives at the two combinations whose pairing
// decides the proof -- e(left, [s]G2) e(right, -G2) = 1 -- or returns false where the proof is malformed; the finish is
// msm_eval (the two combinations on the GPU) and pairing_of.  verify_proof runs one after the other; h2_verify_proofs
// replays every proof of a batch and finishes a random combination of all of them at once (BatchCheck).
// Tags of the terms: the proof's commitments in the order they are registered below -- advice, permutation products,
// the key's fixed and sigma commitments [shared0, shared0 + shared_count), the random polynomial -- then the quotient
// pieces, the opening points and the SRS generator (tag_g0).
struct Replay {
  MsmTerms left, right;
  int shared0 = 0, shared_count = 0, tag_g0 = 0, tags = 0;
};
inline bool replay_proof(ProvingKey& K, const uint8_t* proof, size_t proof_len, const std::vector<Fr>& instance,
                  const Transcript::PointTable* pre, Replay& out) {
  const Circuit& C = *K.circuit;
  const Domain& D = *K.dom;
  const Params& P = *K.params;
  const uint32_t n = D.n;
  const OpeningPlan& L = K.plan;
  const int bf = K.bf, deg = C.degree;
  if (instance.size() > n - (uint32_t)(bf + 1)) return false;
  if (!C.num_instance && !instance.empty()) return false;
  Transcript tr(proof, proof_len);
  if (pre) tr.use_points(*pre);
  tr.common_scalar(K.transcript_repr);
  for (auto& v : instance) tr.common_scalar(v);
  std::vector<G1> advice_c(C.num_advice), z_c(K.sets.size()), h_c(deg - 1);
  for (auto& p : advice_c)
    if (!tr.read_point(&p)) return false;
  const Fr theta = tr.squeeze_challenge(), beta = tr.squeeze_challenge(), gamma = tr.squeeze_challenge();
  (void)theta;
  for (auto& p : z_c)
    if (!tr.read_point(&p)) return false;
  G1 random_c;
  if (!tr.read_point(&random_c)) return false;
  const Fr y = tr.squeeze_challenge();
  for (auto& p : h_c)
    if (!tr.read_point(&p)) return false;
  const Fr x = tr.squeeze_challenge();
  const Fr xn = x.pow_u64(n);
  if (xn == Fr::one()) return false;
  auto lagrange_at = [&](int row) {       // L_row(x) = w^row (x^n - 1) / (n (x - w^row)), row taken mod n
    const Fr wi = row >= 0 ? D.omega.pow_u64((uint64_t)row) : D.omega_inv.pow_u64((uint64_t)(-row));
    return wi * (xn - Fr::one()) * D.n_inv * (x - wi).inv();
  };
  std::vector<Fr> inst_evals;
  for (auto& q : C.instance_queries) {
    Fr acc = Fr::zero();
    for (size_t i = 0; i < instance.size(); i++) acc += instance[i] * lagrange_at((int)i - q.second);
    inst_evals.push_back(acc);
  }
  std::vector<Fr> scalars(L.evals.size());    // in the plan's order; the views below are ranges of it
  for (auto& e : scalars)
    if (!tr.read_scalar(&e)) return false;
  const std::vector<Fr> adv_evals(scalars.begin(), scalars.begin() + L.fixed0),
      fix_evals(scalars.begin() + L.fixed0, scalars.begin() + L.random_at);
  const Fr* sigma_evals = scalars.data() + L.sigma0;
  auto z_ev = [&](size_t i) -> const Fr& { return scalars[L.z0 + 3 * i]; };          // z_i(x)
  auto z_next = [&](size_t i) -> const Fr& { return scalars[L.z0 + 3 * i + 1]; };    // z_i(x w)
  auto z_last = [&](size_t i) -> const Fr& { return scalars[L.z0 + 3 * i + 2]; };    // z_i(x w^-(bf+1)), all sets but the last
  // the vanishing argument
  const Fr l_last = lagrange_at(-(bf + 1)), l_0 = lagrange_at(0);
  Fr l_blind = Fr::zero();
  for (int r = -bf; r < 0; r++) l_blind += lagrange_at(r);
  std::vector<Fr> exprs;
  for (auto& g : C.gates) exprs.push_back(expr_eval(g, adv_evals, fix_evals, inst_evals));
  const Fr delta = fr_delta();
  if (!K.sets.empty()) {
    const size_t ns = K.sets.size();
    exprs.push_back(l_0 * (Fr::one() - z_ev(0)));
    exprs.push_back(l_last * (z_ev(ns - 1).sqr() - z_ev(ns - 1)));
    for (size_t i = 1; i < ns; i++) exprs.push_back(l_0 * (z_ev(i) - z_last(i - 1)));
    auto column_eval = [&](const ColRef& cr) {
      const auto& qs = cr.first == ADVICE ? C.advice_queries : cr.first == FIXED ? C.fixed_queries : C.instance_queries;
      const auto& ev = cr.first == ADVICE ? adv_evals : cr.first == FIXED ? fix_evals : inst_evals;
      for (size_t i = 0; i < qs.size(); i++)
        if (qs[i].first == cr.second && qs[i].second == 0) return ev[i];
      fail(H2_EINVAL, "permutation column is not queried at the current rotation");
    };
    for (size_t i = 0; i < ns; i++) {
      Fr left = z_next(i), right = z_ev(i);
      for (int j : K.sets[i]) {
        const Fr v = column_eval(C.permutation_columns[j]);
        left *= v + beta * sigma_evals[j] + gamma;
        right *= v + delta.pow_u64((uint64_t)j) * beta * x + gamma;
      }
      exprs.push_back((left - right) * (Fr::one() - (l_last + l_blind)));
    }
  }
  Fr folded = Fr::zero();
  for (auto& e : exprs) folded = folded * y + e;
  const Fr expected_h = folded * (xn - Fr::one()).inv();
  const int tag_h0 = C.num_advice + (int)K.sets.size() + (int)K.fixed_commitments.size() + (int)K.sigma_commitments.size() + 1;
  const int tag_open0 = tag_h0 + (int)h_c.size();
  MsmTerms h_msm;
  for (size_t i = h_c.size(); i-- > 0;) {
    h_msm.scale(xn);
    h_msm.append(Fr::one(), h_c[i], tag_h0 + (int)i);
  }
  // the opening queries, in the prover's batching order; commitment -1 = the h combination
  struct VQ { Fr point; int id; Fr eval; };
  std::vector<G1> commitments;
  std::vector<VQ> queries;
  auto reg = [&](const G1& c) { commitments.push_back(c); return (int)commitments.size() - 1; };
  int first[6];                                    // the tag of each kind's polynomial 0, by PolyKind
  first[POLY_ADVICE] = 0;
  for (auto& c : advice_c) reg(c);
  first[POLY_Z] = (int)commitments.size();
  for (auto& c : z_c) reg(c);
  first[POLY_FIXED] = (int)commitments.size();
  for (auto& c : K.fixed_commitments) reg(c);
  first[POLY_SIGMA] = (int)commitments.size();
  for (auto& c : K.sigma_commitments) reg(c);
  first[POLY_RANDOM] = reg(random_c);
  const int id_h = first[POLY_H] = (int)commitments.size();        // not a single point: h_msm
  for (auto& q : L.queries)
    queries.push_back({D.rotate(x, q.rot), first[q.kind] + q.index, q.eval < 0 ? expected_h : scalars[(size_t)q.eval]});
  auto as_msm = [&](int id, const Fr& factor) {
    MsmTerms m;
    if (id == id_h) {
      m = h_msm;
      m.scale(factor);
    } else {
      m.append(factor, commitments[id], id);
    }
    return m;
  };
  MsmTerms& left = out.left;
  MsmTerms& right = out.right;
  out.shared_count = (int)(K.fixed_commitments.size() + K.sigma_commitments.size());
  out.shared0 = out.shared_count ? first[POLY_FIXED] : 0;
  int opening_points = 2;
  if (!L.shplonk) {
    // VerifierGWC (halo2_proofs src/poly/kzg/multiopen/gwc/verifier.rs)
    const Fr v = tr.squeeze_challenge();
    std::vector<Fr> points;
    for (auto& q : queries)
      if (std::find(points.begin(), points.end(), q.point) == points.end()) points.push_back(q.point);
    std::vector<G1> ws(points.size());
    for (auto& w : ws)
      if (!tr.read_point(&w)) return false;
    const Fr u = tr.squeeze_challenge();
    Fr eval_multi = Fr::zero(), up = Fr::one();
    for (size_t pi = 0; pi < points.size(); pi++) {
      Fr vp = Fr::one(), ev = Fr::zero();
      MsmTerms batch;
      for (auto& q : queries)
        if (q.point == points[pi]) {
          batch.add(as_msm(q.id, vp));
          ev += vp * q.eval;
          vp *= v;
        }
      batch.scale(up);
      right.add(batch);
      eval_multi += up * ev;
      right.append(up * points[pi], ws[pi], tag_open0 + (int)pi);
      left.append(up, ws[pi], tag_open0 + (int)pi);
      up *= u;
    }
    opening_points = (int)points.size();
    right.append(-eval_multi, P.g0, tag_open0 + opening_points);
  } else {
    // VerifierSHPLONK (src/poly/kzg/multiopen/shplonk/verifier.rs)
    std::vector<Fr> pts, evs;
    std::vector<uintptr_t> ids;
    for (auto& q : queries) {
      pts.push_back(q.point);
      evs.push_back(q.eval);
      ids.push_back((uintptr_t)q.id);
    }
    const ShplonkSets S = shplonk_sets(pts, evs, ids);
    const Fr y_ch = tr.squeeze_challenge(), v = tr.squeeze_challenge();
    G1 h1, h2;
    if (!tr.read_point(&h1)) return false;
    const Fr u = tr.squeeze_challenge();
    if (!tr.read_point(&h2)) return false;
    MsmTerms outer;
    Fr r_outer = Fr::zero(), vp = Fr::one(), z_0 = Fr::one(), z_0_diff_inv = Fr::one();
    for (size_t gi = 0; gi < S.groups.size(); gi++) {
      const auto& G = S.groups[gi];
      Fr z_diff = Fr::one();
      for (auto& pt : S.super)
        if (std::find(G.points.begin(), G.points.end(), pt) == G.points.end()) z_diff *= u - pt;
      if (gi == 0) {
        for (auto& pt : G.points) z_0 *= u - pt;
        if (z_diff.is_zero()) return false;
        z_0_diff_inv = z_diff.inv();
        z_diff = Fr::one();
      } else {
        z_diff *= z_0_diff_inv;
      }
      MsmTerms inner;
      Fr r_inner = Fr::zero(), yp = Fr::one();
      for (auto& m : G.members) {
        std::vector<Fr> vals;
        for (auto& pt : G.points) vals.push_back(m.evals.at(fr_key(pt)));
        r_inner += yp * horner(interpolate(G.points, vals), u);
        inner.add(as_msm(m.commitment, yp));
        yp *= y_ch;
      }
      inner.scale(vp * z_diff);
      outer.add(inner);
      r_outer += vp * r_inner * z_diff;
      vp *= v;
    }
    outer.append(-r_outer, P.g0, tag_open0 + 2);
    outer.append(-z_0, h1, tag_open0);
    outer.append(u, h2, tag_open0 + 1);
    left.append(Fr::one(), h2, tag_open0 + 1);
    right.add(outer);
  }
  out.tag_g0 = tag_open0 + opening_points;
  out.tags = out.tag_g0 + 1;
  return true;
}

inline uint64_t g_pairing_checks = 0;       // pairing checks made by the two verify entry points (h2_selftest_pairing_checks)

// e(L, [s]G2) e(R, -G2) == 1
inline bool pairing_of(const Params& P, const G1& L, const G1& Rr) {
  bn::G2 neg_g2 = P.g2;
  neg_g2.y = -neg_g2.y;
  g_pairing_checks++;
  return bn::pairing_check({{L, P.s_g2}, {Rr, neg_g2}});
}

inline bool verify_proof(ProvingKey& K, const uint8_t* proof, size_t proof_len, const std::vector<Fr>& instance) {
  const Params& P = *K.params;
  Trace trace("verify");
  Replay r;
  if (!replay_proof(K, proof, proof_len, instance, nullptr, r)) return false;
  if (!bn::g2_on_curve(P.g2) || !bn::g2_on_curve(P.s_g2)) return false;
  trace.mark("transcript replayed");
  Dev d(K.dev->c);
  const std::vector<G1> lr = msm_eval(d, {&r.left, &r.right});
  trace.mark("two MSMs");
  const bool ok = pairing_of(P, lr[0], lr[1]);
  trace.mark("pairing check");
  return ok;
}

// ---- h2_verify_proofs: many proofs of one circuit behind one pairing check --------------------------------------------------------
// one proof's two combinations with equal points added up (by tag): the key's commitments and the SRS generator, which
// every proof of the batch shares, as scalars by index; the proof's own points as terms
struct BatchItem {
  bool replayed = false;
  Fr weight;
  std::vector<std::pair<Fr, G1>> own[2];
  std::vector<Fr> shared[2];           // fixed commitments, sigma commitments, g0
};
inline void fold_replay(const Replay& r, BatchItem& it) {
  const MsmTerms* side[2] = {&r.left, &r.right};
  for (int s = 0; s < 2; s++) {
    std::vector<Fr> acc((size_t)r.tags, Fr::zero());
    std::vector<const G1*> pt((size_t)r.tags, nullptr);
    for (auto& t : side[s]->t) {
      if (t.tag < 0 || t.tag >= r.tags) fail(H2_EINVAL, "verify: a term without a tag");
      acc[(size_t)t.tag] += t.first;
      pt[(size_t)t.tag] = &t.second;
    }
    it.shared[s].assign((size_t)r.shared_count + 1, Fr::zero());
    for (int tag = 0; tag < r.tags; tag++) {
      if (tag >= r.shared0 && tag < r.shared0 + r.shared_count) it.shared[s][(size_t)(tag - r.shared0)] = acc[(size_t)tag];
      else if (tag == r.tag_g0) it.shared[s][(size_t)r.shared_count] = acc[(size_t)tag];
      else if (pt[(size_t)tag] && !pt[(size_t)tag]->inf && !acc[(size_t)tag].is_zero()) it.own[s].push_back({acc[(size_t)tag], *pt[(size_t)tag]});
    }
  }
}

struct BatchCheck {
  ProvingKey& K;
  Dev d;
  Trace& trace;
  std::vector<const G1*> shared_points;
  uint64_t checks = 0;
  BatchCheck(ProvingKey& key, Trace& tr) : K(key), d(key.dev->c), trace(tr) {
    for (auto& c : K.fixed_commitments) shared_points.push_back(&c);
    for (auto& c : K.sigma_commitments) shared_points.push_back(&c);
    shared_points.push_back(&K.params->g0);
  }
  // sum_i w_i (left_i, right_i) over items[lo, hi) of `who`: one small-MSM launch with the two jobs side by side, one pairing
  bool run(const std::vector<BatchItem>& items, const std::vector<size_t>& who, size_t lo, size_t hi) {
    std::vector<std::vector<uint8_t>> pts(2), sc(2);
    for (int s = 0; s < 2; s++) {
      std::vector<Fr> acc(shared_points.size(), Fr::zero());
      auto put = [&](const Fr& k, const G1& g) {
        const size_t at = pts[s].size(), as = sc[s].size();
        pts[s].resize(at + 64);
        sc[s].resize(as + 32);
        memcpy(pts[s].data() + at, g.x.v.v, 32);
        memcpy(pts[s].data() + at + 32, g.y.v.v, 32);
        memcpy(sc[s].data() + as, k.v.v, 32);
      };
      for (size_t q = lo; q < hi; q++) {
        const BatchItem& it = items[who[q]];
        for (auto& t : it.own[s]) put(t.first * it.weight, t.second);
        for (size_t j = 0; j < acc.size(); j++) acc[j] += it.shared[s][j] * it.weight;
      }
      for (size_t j = 0; j < acc.size(); j++)
        if (!acc[j].is_zero() && !shared_points[j]->inf) put(acc[j], *shared_points[j]);
    }
    const std::vector<G1> lr = msm_small_run(d, pts, sc);
    trace.mark("combined msm");
    const bool ok = pairing_of(*K.params, lr[0], lr[1]);
    trace.mark("pairing");
    checks++;
    return ok;
  }
  // items[lo, hi) of `who` failed together (known_bad) or have not been checked: find the bad ones by halving.  A half
  // whose sibling passed after the parent failed is bad without a check of its own.
  void bisect(const std::vector<BatchItem>& items, const std::vector<size_t>& who, size_t lo, size_t hi, bool known_bad, int* ok) {
    if (!known_bad && run(items, who, lo, hi)) {
      for (size_t q = lo; q < hi; q++) ok[who[q]] = 1;
      return;
    }
    if (hi - lo == 1) return;                               // ok stays 0
    const size_t mid = lo + (hi - lo) / 2;
    if (run(items, who, lo, mid)) {
      for (size_t q = lo; q < mid; q++) ok[who[q]] = 1;
      bisect(items, who, mid, hi, true, ok);
    } else {
      bisect(items, who, lo, mid, true, ok);
      bisect(items, who, mid, hi, false, ok);
    }
  }
};

constexpr size_t VERIFY_GROUP = 1024;     // proofs behind one combined check

// proofs [0, count) of one group; ok[] is zero on entry
inline void verify_group(ProvingKey& K, size_t count, const uint8_t* const* proofs, const size_t* lens,
                  const Job* jobs, Rng& rng, int* ok, Trace& trace) {
  const std::vector<uint32_t>& off = K.plan.point_offsets;
  // the compressed points of every proof that lie inside it, proof by proof: one upload, one launch, one download
  std::vector<size_t> first(count + 1, 0);
  std::vector<uint8_t> words;
  for (size_t i = 0; i < count; i++) {
    size_t inside = 0;
    while (inside < off.size() && (size_t)off[inside] + 32 <= lens[i]) inside++;
    first[i + 1] = first[i] + inside;
    for (size_t j = 0; j < inside; j++) words.insert(words.end(), proofs[i] + off[j], proofs[i] + off[j] + 32);
  }
  const size_t total = first[count];
  std::vector<uint8_t> points(64 * total), status(total);
  BatchCheck bc(K, trace);
  if (total) {
    Dev& d = bc.d;
    void* d_in = d.upload(words.data(), words.size());
    void* d_out = d.alloc(64 * total);
    void* d_st = d.alloc(total);
    hip_ok(d.ops->points_decompress(d_in, d_out, d_st, (uint32_t)total, d.s), "points_decompress");
    hip_ok(hipMemcpyAsync(points.data(), d_out, 64 * total, hipMemcpyDeviceToHost, d.s), "hipMemcpyAsync(D2H)");
    hip_ok(hipMemcpyAsync(status.data(), d_st, total, hipMemcpyDeviceToHost, d.s), "hipMemcpyAsync(D2H)");
    d.sync();
    d.release(d_in);
    d.release(d_out);
    d.release(d_st);
  }
  trace.mark("decompress");
  // the weights: 16 bytes per proof, read little-endian; a zero draw becomes 1 (a weight must not cancel its proof)
  std::vector<uint8_t> draw(16 * count);
  rng.fill(draw.data(), draw.size());
  std::vector<BatchItem> items(count);
  std::vector<size_t> who;
  for (size_t i = 0; i < count; i++) {
    uint8_t w[32] = {0};
    memcpy(w, draw.data() + 16 * i, 16);
    items[i].weight = Fr::from_le_bytes_reduce(w);
    if (items[i].weight.is_zero()) items[i].weight = Fr::one();
    Transcript::PointTable pre;
    pre.offsets = off.data();
    pre.count = first[i + 1] - first[i];
    pre.points = points.data() + 64 * first[i];
    pre.status = status.data() + first[i];
    Replay r;
    if (!replay_proof(K, proofs[i], lens[i], jobs[i].public_input, &pre, r)) continue;
    fold_replay(r, items[i]);
    items[i].replayed = true;
    who.push_back(i);
  }
  trace.mark("replay");
  if (!who.empty()) bc.bisect(items, who, 0, who.size(), false, ok);
  if (trace.on) fprintf(stderr, "[h2 %s] checks %llu of %zu proofs (%zu replayed, %zu points)\n", trace.what,
                        (unsigned long long)bc.checks, count, who.size(), total);
}

}  // namespace product
}  // namespace h2

namespace h2 {

// Blake2bRead::read_point: 32 bytes, x little-endian with the parity of y in bit 6 and the identity flag in bit 7
bool h2::Transcript::read_point(G1* p) {
  const uint8_t* src = take32();
  if (!src) return false;
  if (pre_.count) {                          // decompressed ahead of the replay: the same decision, the same point
    const size_t at = (size_t)(src - in_);
    const uint32_t* hit = std::lower_bound(pre_.offsets, pre_.offsets + pre_.count, at,
                                           [](uint32_t o, size_t v) { return (size_t)o < v; });
    if (hit != pre_.offsets + pre_.count && (size_t)*hit == at) {
      const size_t i = (size_t)(hit - pre_.offsets);
      if (pre_.status[i] != 0) return false;
      G1 g = product::affine_from_raw(pre_.points + 64 * i);
      g.inf = false;
      common_point(g);
      *p = g;
      return true;
    }
  }
  uint8_t b[32];
  memcpy(b, src, 32);
  const int sign = (b[31] >> 6) & 1, inf = (b[31] >> 7) & 1;
  b[31] &= 0x3F;
  Fq x;
  if (!Fq::from_le_bytes_canonical(b, &x)) return false;
  G1 g;
  if (inf || (x.is_zero() && sign == 0)) {
    // the reference's Blake2bRead::read_point absorbs the point through common_point, which refuses the point at
    // infinity ("cannot write points at infinity to the transcript"): verify_proof returns Err for such a proof
    return false;
  } else {
    const Fq y2 = x * x * x + Fq::from_u64(3);
    // q = 3 mod 4: a square root is y2^((q + 1) / 4)
    uint64_t e[4];
    for (int i = 0; i < 4; i++) e[i] = (uint64_t)BN254_FQ::P(2 * i) | ((uint64_t)BN254_FQ::P(2 * i + 1) << 32);
    e[0] += 1;                                            // no carry: the low word of q ends in ...47
    for (int i = 0; i < 4; i++) e[i] = (e[i] >> 2) | (i < 3 ? e[i + 1] << 62 : 0);
    Fq y = y2.pow_limbs(e);
    if (!(y * y == y2)) return false;
    if ((y.is_odd() ? 1 : 0) != sign) y = -y;
    g.x = x;
    g.y = y;
    g.inf = false;
  }
  common_point(g);
  *p = g;
  return true;
}

}  // namespace h2
