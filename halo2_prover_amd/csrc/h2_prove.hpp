// h2_prove.hpp -- create_proof: one proof's state, its phases in the reference's order,
// and the two openings.
#pragma once
#include "h2_keygen.hpp"

namespace h2 {
namespace product {

// ---- create_proof ------------------------------------------------------------------------------
struct Query {
  Fr point;
  Col poly;
  Fr eval;
};

// The host side of ProverSHPLONK::create_proof (prover.py _shplonk_open), shared by the single and
// the lockstep prover: the rotation sets, then per set the y-power combination of its members with the low coefficients
// to subtract from it (the combined remainders) and the set's power of v; after u, the terms of L(X).
struct ShplonkOpening {
  Fr y, v;
  ShplonkSets S;
  std::vector<std::vector<std::vector<Fr>>> rems;      // [set][member]: the remainder through the member's evaluations
  struct GroupWork {
    std::vector<std::pair<Col, Fr>> terms;             // sum_j y^j f_j
    std::vector<Fr> rsum;                              // sum_j y^j r_j
    Fr vp;                                             // v^set
  };
  std::vector<GroupWork> groups;
  ShplonkOpening(Transcript& tr, const std::vector<Query>& queries) {
    y = tr.squeeze_challenge();
    v = tr.squeeze_challenge();
    std::vector<Fr> pts, evs;
    std::vector<uintptr_t> ids;
    for (auto& q : queries) {
      pts.push_back(q.point);
      evs.push_back(q.eval);
      ids.push_back((uintptr_t)q.poly);
    }
    S = shplonk_sets(pts, evs, ids);
    rems.resize(S.groups.size());
    Fr vp = Fr::one();
    for (size_t gi = 0; gi < S.groups.size(); gi++) {
      const auto& G = S.groups[gi];
      GroupWork w;
      w.rsum.assign(G.points.size(), Fr::zero());
      w.vp = vp;
      Fr yp = Fr::one();
      for (auto& m : G.members) {
        std::vector<Fr> vals;
        for (auto& pt : G.points) vals.push_back(m.evals.at(fr_key(pt)));
        const std::vector<Fr> r = interpolate(G.points, vals);
        rems[gi].push_back(r);
        w.terms.push_back({m.poly, yp});
        for (size_t i = 0; i < r.size(); i++) w.rsum[i] += yp * r[i];
        yp *= y;
      }
      groups.push_back(std::move(w));
      vp *= v;
    }
  }
  // L(X) = sum_i v^i z_i (sum_j y^j (f_ij(X) - r_ij(u))) - Z_T(u) h(X): its terms, the constant to subtract and 1 / z_0
  struct Final {
    std::vector<std::pair<Col, Fr>> terms;
    Fr lconst, z0_inv;
  };
  Final finish(const Fr& u, Col h) const {
    Final f;
    Fr zt = Fr::one();
    for (auto& pt : S.super) zt *= u - pt;
    f.lconst = Fr::zero();
    Fr z0 = Fr::zero(), vp = Fr::one();
    for (size_t gi = 0; gi < S.groups.size(); gi++) {
      const auto& G = S.groups[gi];
      Fr z_i = Fr::one();
      for (auto& pt : S.super)
        if (std::find(G.points.begin(), G.points.end(), pt) == G.points.end()) z_i *= u - pt;
      if (gi == 0) z0 = z_i;
      Fr yp = Fr::one();
      for (size_t mi = 0; mi < G.members.size(); mi++) {
        f.terms.push_back({G.members[mi].poly, vp * z_i * yp});
        f.lconst += vp * z_i * yp * horner(rems[gi][mi], u);
        yp *= y;
      }
      vp *= v;
    }
    f.terms.push_back({h, -zt});
    f.z0_inv = z0.inv();
    return f;
  }
};

inline void shplonk_open(Transcript& tr, Dev& d, const Params& P, uint32_t n, const std::vector<Query>& queries) {
  const ShplonkOpening O(tr, queries);
  Col h = d.col(n), acc = d.col(n), quo = d.col(n);
  for (size_t gi = 0; gi < O.groups.size(); gi++) {
    const auto& w = O.groups[gi];
    d.lincomb(acc, n, w.terms);
    Col d_r = d.upload_frs(w.rsum);
    launch("sub_prefix_kernel", pk::sub_prefix_kernel, dim3(1), dim3(64), d.s, acc, d_r, (uint32_t)w.rsum.size());
    // divide by prod (X - p): one synthetic division per point, ping-ponging two buffers (the quotient keeps the
    // column's length, its top coefficients are zero)
    Col src = acc, dst = quo;
    for (auto& pt : O.S.groups[gi].points) {
      d.scan_batch(0, n, {src}, {dst}, {pt});
      std::swap(src, dst);
    }
    d.lincomb(h, n, gi == 0 ? std::vector<std::pair<Col, Fr>>{{src, w.vp}}
                            : std::vector<std::pair<Col, Fr>>{{h, Fr::one()}, {src, w.vp}});
  }
  tr.write_point(commit(d, P, h, n, 1, false)[0]);
  const Fr u = tr.squeeze_challenge();
  const ShplonkOpening::Final L = O.finish(u, h);    // then / (X - u) / z_0
  d.lincomb(acc, n, L.terms);
  {
    std::vector<Fr> c0(1, L.lconst);
    Col d_c = d.upload_frs(c0);
    launch("sub_prefix_kernel", pk::sub_prefix_kernel, dim3(1), dim3(64), d.s, acc, d_c, 1u);
  }
  d.scan_batch(0, n, {acc}, {quo}, {u});
  launch("scale_range_kernel", pk::scale_range_kernel, dim3((n + 255) / 256), dim3(256), d.s, quo, 0u, n, L.z0_inv.v);
  tr.write_point(commit(d, P, quo, n, 1, false)[0]);
}

// ProverGWC::create_proof: one witness polynomial per distinct point, the v-power combination of everything opened there
inline void gwc_open(Transcript& tr, Dev& d, const Params& P, uint32_t n, const std::vector<Query>& queries) {
  const Fr v = tr.squeeze_challenge();
  std::vector<Fr> points;
  for (auto& q : queries)
    if (std::find(points.begin(), points.end(), q.point) == points.end()) points.push_back(q.point);
  Col witnesses = d.col(points.size() * (size_t)n);
  Col accs = d.col(points.size() * (size_t)n);
  {
    std::vector<Col> in, out;
    for (size_t pi = 0; pi < points.size(); pi++) {
      std::vector<std::pair<Col, Fr>> t;
      Fr vp = Fr::one();
      for (auto& q : queries)
        if (q.point == points[pi]) {
          t.push_back({q.poly, vp});
          vp *= v;
        }
      d.lincomb(accs + 2 * pi * (size_t)n, n, t);
      in.push_back(accs + 2 * pi * (size_t)n);
      out.push_back(witnesses + 2 * pi * (size_t)n);
    }
    d.scan_batch(0, n, in, out, points);          // the four synthetic divisions side by side
  }
  for (auto& pt : commit(d, P, witnesses, n, points.size(), false)) tr.write_point(pt);
}

// a witness's advice columns (not yet blinded) behind the checks a prover makes before it draws or enqueues anything
inline std::vector<SparseCol> synthesize_checked(const Circuit& C, const std::vector<Fr>& public_input, uint32_t n, int bf) {
  if (public_input.size() > n - (uint32_t)(bf + 1)) fail(H2_EINVAL, "instance too long");
  if (!C.num_instance && !public_input.empty()) fail(H2_EINVAL, "circuit has no instance column");
  std::vector<SparseCol> adv = C.synthesize_advice();
  for (auto& col : adv)
    if (!col.empty() && col.rbegin()->first >= n - (uint32_t)(bf + 1)) fail(H2_EINVAL, "k too small for this circuit");
  return adv;
}

// One proof: its state, and its phases in the order create_proof calls them.  Every phase enqueues on the main stream
// d.s unless it says otherwise; the RNG draws (the discarded Blinds included) and the transcript writes are the
// reference's, in its order.
struct Proving {
  ProvingKey& K;
  const Circuit& C;
  const std::vector<Fr>& public_input;
  Rng& rng;
  Trace trace{"prove"};
  const Domain& D;
  const Params& P;
  Dev d;
  const uint32_t n, en;
  const int bf, deg;
  const size_t na, ni, nz, nf, np;
  Transcript tr;
  // Lagrange columns of this proof: advice | instance | z
  // ... | random polynomial (coefficient form; it sits behind the z columns so that both share one MSM launch)
  Col lag = nullptr, advice_values = nullptr, instance_values = nullptr, z_values = nullptr, random_poly = nullptr;
  // their coefficient and extended-coset forms (advice | instance | z), made on the second stream
  Col polys = nullptr, ext = nullptr, advice_polys = nullptr, z_polys = nullptr;
  hipStream_t side = nullptr;
  const Fr delta = fr_delta();
  Fr theta, beta, gamma, y, x;                // the challenges, once drawn
  Col h_pieces = nullptr;                     // deg - 1 pieces of n coefficients, contiguous
  Col h_poly = nullptr;
  std::vector<Fr> evals;                      // in the plan's order, then h(x) when the opening is SHPLONK's

  Proving(ProvingKey& key, const Circuit& circuit, const std::vector<Fr>& instance, Rng& r)
      : K(key), C(circuit), public_input(instance), rng(r), D(*key.dom), P(*key.params), d(key.dev->c), n(D.n), en(D.en),
        bf(key.bf), deg(circuit.degree), na((size_t)circuit.num_advice), ni((size_t)circuit.num_instance), nz(key.sets.size()),
        nf(key.nf()), np(key.np()) {}

  void upload_instance_and_advice() {
    std::vector<SparseCol> adv = synthesize_checked(C, public_input, n, bf);
    tr.common_scalar(K.transcript_repr);
    lag = d.col((na + ni + nz + 1) * (size_t)n);
    advice_values = lag;
    instance_values = lag + 2 * na * (size_t)n;
    z_values = lag + 2 * (na + ni) * (size_t)n;
    random_poly = lag + 2 * (na + ni + nz) * (size_t)n;
    if (ni) {
      std::vector<SparseCol> inst(1);
      for (size_t i = 0; i < public_input.size(); i++) inst[0][(uint32_t)i] = public_input[i];
      d.fill_sparse(instance_values, n, inst);
      for (auto& v : public_input) tr.common_scalar(v);
    }
    // advice: blind the last bf + 1 rows
    for (auto& col : adv)
      for (uint32_t row = n - (bf + 1); row < n; row++) col[row] = rng.fr_random();
    for (size_t j = 0; j < adv.size(); j++) (void)rng.fr_random();       // the Blind of each commitment (unused by KZG)
    d.fill_sparse(advice_values, n, adv);
    trace.mark("witness uploaded");
  }

  // Lagrange -> coefficient -> extended coset of the advice and instance columns: they wait for no challenge, so they
  // run on the context's second stream beside the commit phases (whose MSM tails leave the chip mostly idle); the
  // permutation products' follow once those exist; the main stream takes everything back before the quotient
  void commit_advice() {
    polys = d.col((na + ni + nz) * (size_t)n);
    ext = d.col((na + ni + nz) * (size_t)en);
    side = d.side();
    PendingCommit pc = commit_begin(d, P, advice_values, n, na, true);
    d.wait_msm_tail(side);                       // (the tail event lies behind the witness upload on the main stream)
    hip_ok(hipMemcpyAsync(polys, lag, (na + ni) * (size_t)n * 32, hipMemcpyDeviceToDevice, side), "hipMemcpyAsync(D2D)");
    d.ntt(polys, na + ni, D.omega_inv, D.k, &D.n_inv, side);
    coeff_to_extended(d, D, polys, na + ni, ext, side);
    for (auto& pt : commit_finish(d, pc)) tr.write_point(pt);
    trace.mark("advice committed");
    theta = tr.squeeze_challenge();
    beta = tr.squeeze_challenge();
    gamma = tr.squeeze_challenge();
  }

  Col values_of(const ColRef& cr) const {
    if (cr.first == ADVICE) return advice_values + 2 * (size_t)cr.second * n;
    if (cr.first == FIXED) return K.fixed_values + 2 * (size_t)cr.second * n;
    return instance_values + 2 * (size_t)cr.second * n;
  }

  // permutation grand products
  void permutation_products() {
    if (nz) {
      // every set's ratio column in ONE launch sequence (they only need beta and gamma), then one read-back of the
      // sets' last usable products: z_i = (prod_{s < i} tail_s) * prefix_i, blinding rows drawn set by set
      Col ratio = d.col(nz * (size_t)n);
      for (size_t s0 = 0; s0 < nz; s0 += pk::PERM_MAX_SETS) {
        const size_t cnt = std::min<size_t>(pk::PERM_MAX_SETS, nz - s0);
        pk::PermBatch B{};
        for (size_t q = 0; q < cnt; q++) {
          pk::PermArgs& A = B.set[q];
          const size_t si = s0 + q;
          A.ncols = (int)K.sets[si].size();
          if (A.ncols > pk::PERM_MAX_COLS) fail(H2_EINVAL, "permutation set too wide");
          for (int t = 0; t < A.ncols; t++) {
            const int j = K.sets[si][t];
            A.value[t] = values_of(C.permutation_columns[j]);
            A.sigma[t] = K.sigma_values + 2 * (size_t)j * n;
            A.beta_delta[t] = (beta * delta.pow_u64((uint64_t)j)).v;
          }
          A.beta = beta.v;
          A.gamma = gamma.v;
        }
        launch("perm_ratio_kernel", pk::perm_ratio_kernel, dim3((n / pk::PERM_RUN + 255) / 256 + 1, (unsigned)cnt), dim3(256), d.s,
               B, K.omega_col, ratio + 2 * s0 * (size_t)n, n);
      }
      {
        std::vector<Col> in, out;
        for (size_t si = 0; si < nz; si++) {
          in.push_back(ratio + 2 * si * (size_t)n);
          out.push_back(z_values + 2 * si * (size_t)n);
        }
        d.scan_batch(1, n, in, out, {});
      }
      // the products over the usable rows (row n - bf - 1 of every prefix column): one gather, one copy back
      Col tails_d = d.col(nz);
      for (size_t si = 0; si < nz; si++) d.copy(tails_d + 2 * si, z_values + 2 * (si * (size_t)n + (n - bf - 1)), 32);
      const std::vector<Fr> tails = d.download_frs(tails_d, nz);
      Fr last_z = Fr::one();
      for (size_t si = 0; si < nz; si++) {
        Col z = z_values + 2 * si * (size_t)n;
        if (!(last_z == Fr::one()))
          launch("scale_range_kernel", pk::scale_range_kernel, dim3((n + 255) / 256), dim3(256), d.s, z, 0u, n, last_z.v);
        std::vector<Fr> blind(bf);
        for (int t = 0; t < bf; t++) blind[t] = rng.fr_random();
        Col d_blind = d.upload_frs(blind);
        d.copy(z + 2 * (size_t)(n - bf), d_blind, (size_t)bf * 32);
        last_z = last_z * tails[si];
        (void)rng.fr_random();
      }
      d.release(ratio);
    }
    trace.mark("grand products built");
  }

  // the vanishing argument's random polynomial: one ChaCha20 seed, n sequential draws.  It comes from the RNG, not
  // from the transcript, so its commitment (over g) is computed in the launch of the permutation products' (over
  // g_lagrange); the transcript still receives the points in the reference's order
  void random_poly_and_commit() {
    uint8_t seed[32];
    rng.fill(seed, 32);
    uint32_t key[8];
    memcpy(key, seed, 32);
    hip_ok(d.ops->chacha20_scalars(random_poly, n, 0, key, d.s), "chacha20_scalars");
    (void)rng.fr_random();
    PendingCommit pc = commit_begin(d, P, z_values, n, nz + 1, true, nz);
    if (nz) {
      d.wait_msm_tail(side);                     // the z columns (blinding rows included) are final before that MSM
      Col zp = polys + 2 * (na + ni) * (size_t)n;
      hip_ok(hipMemcpyAsync(zp, z_values, nz * (size_t)n * 32, hipMemcpyDeviceToDevice, side), "hipMemcpyAsync(D2D)");
      d.ntt(zp, nz, D.omega_inv, D.k, &D.n_inv, side);
      coeff_to_extended(d, D, zp, nz, ext + 2 * (na + ni) * (size_t)en, side);
    }
    for (auto& pt : commit_finish(d, pc)) tr.write_point(pt);
    trace.mark("grand products + random poly committed");
  }

  // the quotient: one program over every extended column
  void quotient() {
    advice_polys = polys;
    z_polys = polys + 2 * (na + ni) * (size_t)n;
    y = tr.squeeze_challenge();
    d.order(side, d.s, 2);                       // every coefficient and extended form is needed from here on
    Col h_ext = d.col(en);
    {
      const ColumnMap& M = K.cmap;
      std::vector<const U128*> ptrs(M.count);
      std::vector<uint32_t> masks(M.count, en - 1);
      for (size_t j = 0; j < na; j++) ptrs[M.advice0 + j] = ext + 2 * j * (size_t)en;
      for (size_t j = 0; j < nf; j++) ptrs[M.fixed0 + j] = K.fixed_ext + 2 * j * (size_t)en;
      for (size_t j = 0; j < ni; j++) ptrs[M.instance0 + j] = ext + 2 * (na + j) * (size_t)en;
      for (size_t j = 0; j < np; j++) ptrs[M.sigma0 + j] = K.sigma_ext + 2 * j * (size_t)en;
      for (size_t j = 0; j < nz; j++) ptrs[M.z0 + j] = ext + 2 * (na + ni + j) * (size_t)en;
      ptrs[M.l0] = K.basis_ext;
      ptrs[M.l_last] = K.basis_ext + 2 * (size_t)en;
      ptrs[M.l_blind] = K.basis_ext + 4 * (size_t)en;
      ptrs[M.xcol] = K.xcol_ext;
      ptrs[M.tinv] = K.tinv;
      masks[M.tinv] = (1u << (D.ext_k - D.k)) - 1;
      std::vector<Fr> consts = K.prog.consts;
      consts[K.c_y] = y;
      consts[K.c_beta] = beta;
      consts[K.c_gamma] = gamma;
      for (size_t j = 0; j < np; j++) consts[K.c_beta_delta[j]] = beta * delta.pow_u64((uint64_t)j);
      expr_launch(d, K.prog, K.d_code, ptrs, masks, std::move(consts), h_ext, en / n, en);
    }
    d.release(ext);
    // extended -> coefficients: inverse NTT with 1 / 2^ext_k, un-shift the coset, keep n (deg - 1) coefficients
    d.ntt(h_ext, 1, D.ext_omega_inv, D.ext_k, &D.en_inv);
    const uint32_t hlen = n * (uint32_t)(deg - 1);
    launch("coset_shrink_kernel", pk::coset_shrink_kernel, dim3((hlen + 255) / 256), dim3(256), d.s, h_ext, hlen, D.zeta_inv.v,
           D.zeta_inv.sqr().v);
    h_pieces = h_ext;
    trace.mark("quotient enqueued");
    for (auto& pt : commit(d, P, h_pieces, n, (size_t)(deg - 1), false)) tr.write_point(pt);
    trace.mark("quotient committed");
    for (int t = 0; t < deg - 1; t++) (void)rng.fr_random();
  }

  Col poly_of(const Opening& p) const {
    switch (p.kind) {
      case POLY_ADVICE: return advice_polys + 2 * (size_t)p.index * n;
      case POLY_FIXED: return K.fixed_polys + 2 * (size_t)p.index * n;
      case POLY_SIGMA: return K.sigma_polys + 2 * (size_t)p.index * n;
      case POLY_Z: return z_polys + 2 * (size_t)p.index * n;
      case POLY_RANDOM: return random_poly;
      default: return h_poly;
    }
  }

  // evaluations at x and its rotations, in the plan's order
  void evaluate() {
    const OpeningPlan& L = K.plan;
    x = tr.squeeze_challenge();
    std::vector<std::pair<Col, Fr>> jobs;
    for (auto& e : L.evals) jobs.push_back({poly_of(e), D.rotate(x, e.rot)});
    // h(X) = sum_i x^(n i) h_i(X), opened at x too
    h_poly = d.col(n);
    {
      const Fr xn = x.pow_u64(n);
      std::vector<std::pair<Col, Fr>> t;
      Fr p = Fr::one();
      for (int i = 0; i < deg - 1; i++) {
        t.push_back({h_pieces + 2 * (size_t)i * n, p});
        p *= xn;
      }
      d.lincomb(h_poly, n, t);
    }
    if (L.shplonk) jobs.push_back({h_poly, x});
    evals = d.evaluate(jobs, n);
    for (size_t i = 0; i < L.evals.size(); i++) tr.write_scalar(evals[i]);
    trace.mark("evaluations");
  }

  // the opening queries in the prover's batching order, and the multi-open over them
  void open() {
    const OpeningPlan& L = K.plan;
    std::vector<Query> queries;
    for (auto& q : L.queries) {
      Fr value = Fr::zero();                     // h in a GWC proof: no value was computed, and that prover reads none
      if (q.eval >= 0) value = evals[(size_t)q.eval];
      else if (L.shplonk) value = evals.back();
      queries.push_back({D.rotate(x, q.rot), poly_of(q), value});
    }
    if (L.shplonk) {
      shplonk_open(tr, d, P, n, queries);
      return;
    }
    gwc_open(tr, d, P, n, queries);
    trace.mark("openings committed");
  }
};

inline std::vector<uint8_t> create_proof(ProvingKey& K, const Circuit& C, const std::vector<Fr>& public_input, Rng& rng) {
  Proving p(K, C, public_input, rng);
  p.upload_instance_and_advice();
  p.commit_advice();
  p.permutation_products();
  p.random_poly_and_commit();
  p.quotient();
  p.evaluate();
  p.open();
  return p.tr.bytes();
}

}  // namespace product
}  // namespace h2
