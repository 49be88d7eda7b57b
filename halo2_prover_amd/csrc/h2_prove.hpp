// h2_prove.hpp -- create_proof for N witnesses of one circuit in lockstep, behind both
// h2_generate_proof (N = 1) and h2_generate_proofs: the phases in the reference's order, each device step issued once for
// the batch, then one transcript step per proof on the host, and the two openings.  Proof p draws from its own RNG in
// the reference's order (the discarded Blinds included) and keeps its own transcript, so its bytes do not depend on its
// neighbours.
//
// Columns are kind-major, so that a batch's columns of one kind are one evenly strided block (one MSM, one NTT):
//   Lagrange      N na advice (proof p's at p na) | N ni instance | N nz permutation products | N random polynomials
//   coefficients  N na | N ni | N nz         extended  the same order, en rows each
// (the random polynomials, in coefficient form, sit behind the z columns so that both can share one MSM launch)
#pragma once
#include "h2_keygen.hpp"
#include "h2_tune.hpp"

namespace h2 {
namespace product {

struct Query {
  Fr point;
  Col poly;
  Fr eval;
};

// The host side of ProverSHPLONK::create_proof (prover.py _shplonk_open) for one proof: the rotation
// sets, then per set the y-power combination of its members with the low coefficients to subtract from it (the combined
// remainders) and the set's power of v; after u, the terms of L(X).
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

// a witness's advice columns (not yet blinded) behind the checks a prover makes before it draws or enqueues anything
inline std::vector<SparseCol> synthesize_checked(const Circuit& C, const std::vector<Fr>& public_input, uint32_t n, int bf) {
  if (public_input.size() > n - (uint32_t)(bf + 1)) fail(H2_EINVAL, "instance too long");
  if (!C.num_instance && !public_input.empty()) fail(H2_EINVAL, "circuit has no instance column");
  std::vector<SparseCol> adv = C.synthesize_advice();
  for (auto& col : adv)
    if (!col.empty() && col.rbegin()->first >= n - (uint32_t)(bf + 1)) fail(H2_EINVAL, "k too small for this circuit");
  return adv;
}

inline size_t g_prove_group = PROVE_GROUP;

// one witness of the batch: what the entry point parsed and synthesised before anything was enqueued
struct Witness {
  const std::vector<Fr>* public_input;
  std::vector<SparseCol> advice;              // synthesised, not yet blinded
  Rng rng;
};

// A group of proofs: its state, and its phases in the order run() calls them.  Every phase enqueues on the main stream
// d.s unless it says otherwise; the RNG draws (the discarded Blinds included) and the transcript writes are the
// reference's, in its order, proof by proof.
struct Proving {
  ProvingKey& K;
  std::vector<Witness>& items;              // this group's
  const size_t N;
  Trace& trace;
  const Domain& D;
  const Params& P;
  Dev d;
  const uint32_t n, en;
  const int bf, deg;
  const size_t na, ni, nz, nf, np;
  const Fr delta = fr_delta();
  struct Proof {
    Transcript tr;
    Fr theta, beta, gamma, y, x;
    std::vector<Fr> evals;                    // in the plan's order, then h(x) when the opening is SHPLONK's
  };
  std::vector<Proof> proofs;
  // the Lagrange columns (advice | instance | z | random polynomials), then their coefficient and extended-coset forms
  // (advice | instance | z), made on the second stream
  Col lag = nullptr, advice_values = nullptr, instance_values = nullptr, z_values = nullptr, random_polys = nullptr;
  Col polys = nullptr, ext = nullptr, advice_polys = nullptr, z_polys = nullptr;
  Col h_pieces = nullptr;                     // N x (deg - 1) pieces of n coefficients, contiguous
  Col h_polys = nullptr;                      // N columns
  hipStream_t side = nullptr;

  Proving(ProvingKey& key, std::vector<Witness>& group, Trace& t)
      : K(key), items(group), N(group.size()), trace(t), D(*key.dom), P(*key.params), d(key.dev->c), n(D.n), en(D.en), bf(key.bf),
        deg(key.circuit->degree), na((size_t)key.circuit->num_advice), ni((size_t)key.circuit->num_instance), nz(key.sets.size()),
        nf(key.nf()), np(key.np()), proofs(group.size()) {}

  Col column(Col base, size_t index, size_t rows) const { return base + 2 * index * rows; }

  struct Lincombs {
    std::vector<pk::LincombJob> jobs;
    std::vector<pk::LincombTerm> terms;
    void add(Col out, const std::vector<std::pair<Col, Fr>>& t) {
      jobs.push_back({out, (uint32_t)terms.size(), (uint32_t)t.size()});
      for (auto& e : t) terms.push_back({e.first, e.second.v});
    }
  };
  // The launches of a phase between two read-backs, in two passes.  The kernels read their jobs, terms and constants
  // from HBM: the first pass gathers a phase's tables on the host and notes each launch as a plain record (which kernel,
  // where its tables sit, how many jobs); run() uploads the tables ONCE and issues the records in order against that one
  // buffer (an upload per table cost one Collatz proof ~50 us against arguments passed by value)
  struct Steps {
    enum Kind { LINCOMB, SCALE, SUB_PREFIX, SCAN, BLINDS };
    struct Step {
      Kind kind;
      size_t a = 0, b = 0;                      // offsets of the step's tables
      unsigned count = 0;                       // jobs (grid.y)
      std::vector<Col> in, out;                 // SCAN: Dev::scan_batch's arguments
      std::vector<Fr> z;
    };
    Proving& B;
    std::vector<uint8_t> tables;
    std::vector<Step> steps;
    explicit Steps(Proving& batch) : B(batch) {}
    size_t room(size_t bytes) {
      const size_t at = (tables.size() + 31) & ~(size_t)31;
      tables.resize(at + bytes);
      return at;
    }
    template <class T>
    size_t put(const std::vector<T>& v) {
      const size_t at = room(v.size() * sizeof(T));
      if (!v.empty()) memcpy(tables.data() + at, v.data(), v.size() * sizeof(T));
      return at;
    }
    size_t put_frs(const std::vector<Fr>& v) {
      const size_t at = room(v.size() * 32);
      for (size_t i = 0; i < v.size(); i++) memcpy(tables.data() + at + 32 * i, v[i].v.v, 32);
      return at;
    }
    Step& add(Kind kind, size_t a, size_t b, size_t count) {
      steps.emplace_back();
      Step& st = steps.back();
      st.kind = kind;
      st.a = a;
      st.b = b;
      st.count = (unsigned)count;
      return st;
    }
    // out_j = sum_t c_t a_t, grid.y = job
    void lincomb(const Lincombs& L) {
      if (!L.jobs.empty()) add(LINCOMB, put(L.jobs), put(L.terms), L.jobs.size());
    }
    // column j *= its constant, grid.y = job
    void scale(const std::vector<pk::ScaleJob>& jobs) {
      if (!jobs.empty()) add(SCALE, put(jobs), 0, jobs.size());
    }
    // column j -= its values (the low coefficients of a remainder), grid.y = job
    void sub_prefix(const std::vector<Col>& cols, const std::vector<std::vector<Fr>>& values) {
      std::vector<pk::SubPrefixJob> jobs;
      std::vector<Fr> table;
      for (size_t j = 0; j < cols.size(); j++) {
        jobs.push_back({cols[j], (uint32_t)table.size(), (uint32_t)values[j].size()});
        table.insert(table.end(), values[j].begin(), values[j].end());
      }
      if (!jobs.empty()) add(SUB_PREFIX, put(jobs), put_frs(table), jobs.size());
    }
    // Dev::scan_batch in its place among the steps (its arguments travel by value, eight jobs a launch)
    void scan(const std::vector<Col>& in, const std::vector<Col>& out, const std::vector<Fr>& z) {
      Step& st = add(SCAN, 0, 0, in.size());
      st.in = in;
      st.out = out;
      st.z = z;
    }
    // the blinding rows (bf each) of the `columns` permutation products
    void blinds(const std::vector<Fr>& values, size_t columns) { add(BLINDS, put_frs(values), 0, columns); }
    void run() {
      const uint8_t* t = tables.empty() ? nullptr : (const uint8_t*)B.d.upload(tables.data(), tables.size());
      const uint32_t n = B.n;
      hipStream_t s = B.d.s;
      for (const Step& st : steps) switch (st.kind) {
          case LINCOMB:
            launch("lincomb_batch_kernel", pk::lincomb_batch_kernel, dim3((n + 255) / 256, st.count), dim3(256), s,
                   (const pk::LincombJob*)(t + st.a), (const pk::LincombTerm*)(t + st.b), n);
            break;
          case SCALE:
            launch("scale_kernel", pk::scale_kernel, dim3((n + 255) / 256, st.count), dim3(256), s,
                   (const pk::ScaleJob*)(t + st.a), n);
            break;
          case SUB_PREFIX:
            launch("sub_prefix_kernel", pk::sub_prefix_kernel, dim3(1, st.count), dim3(64), s,
                   (const pk::SubPrefixJob*)(t + st.a), (const U128*)(t + st.b));
            break;
          case SCAN:
            B.d.scan_batch(n, st.in, st.out, st.z);
            break;
          case BLINDS:
            B.copy_strided(B.z_values + 2 * (size_t)(n - B.bf), (size_t)n * 32, t + st.a, (size_t)B.bf * 32, (size_t)B.bf * 32,
                           st.count);
            break;
        }
      steps.clear();
      tables.clear();
    }
  };
  // `rows` x `bytes` between two evenly strided places on the device
  void copy_strided(void* dst, size_t dst_pitch, const void* src, size_t src_pitch, size_t bytes, size_t rows) {
    hip_ok(hipMemcpy2DAsync(dst, dst_pitch, src, src_pitch, bytes, rows, hipMemcpyDeviceToDevice, d.s), "hipMemcpy2DAsync(D2D)");
  }

  void upload_instances_and_advice() {
    lag = d.col((N * (na + ni + nz + 1)) * (size_t)n);
    advice_values = lag;
    instance_values = column(lag, N * na, n);
    z_values = column(lag, N * (na + ni), n);
    random_polys = column(lag, N * (na + ni + nz), n);
    std::vector<SparseCol> inst(N * ni), adv;
    for (size_t p = 0; p < N; p++) {
      Witness& it = items[p];
      Transcript& tr = proofs[p].tr;
      tr.common_scalar(K.transcript_repr);
      if (ni) {
        for (size_t i = 0; i < it.public_input->size(); i++) inst[p * ni][(uint32_t)i] = (*it.public_input)[i];
        for (auto& v : *it.public_input) tr.common_scalar(v);
      }
      // blind the last bf + 1 rows, then the Blind of each commitment (unused by KZG)
      for (auto& col : it.advice)
        for (uint32_t row = n - (bf + 1); row < n; row++) col[row] = it.rng.fr_random();
      for (size_t j = 0; j < it.advice.size(); j++) (void)it.rng.fr_random();
      for (auto& col : it.advice) adv.push_back(std::move(col));
    }
    if (ni) d.fill_sparse(instance_values, n, inst);
    d.fill_sparse(advice_values, n, adv);
    trace.mark("witnesses uploaded");
  }

  // Lagrange -> coefficient -> extended coset of the advice and instance columns: they wait for no challenge, so they
  // run on the context's second stream beside the commit phases (whose MSM tails leave the chip mostly idle); the
  // permutation products' follow once those exist; the main stream takes everything back before the quotient
  void commit_advice() {
    polys = d.col(N * (na + ni + nz) * (size_t)n);
    ext = d.col(N * (na + ni + nz) * (size_t)en);
    side = d.side();
    PendingCommit pc = commit_begin(d, P, advice_values, n, N * na, true);
    d.wait_msm_tail(side);                       // (the tail event lies behind the witness upload on the main stream)
    hip_ok(hipMemcpyAsync(polys, lag, N * (na + ni) * (size_t)n * 32, hipMemcpyDeviceToDevice, side), "hipMemcpyAsync(D2D)");
    d.ntt(polys, N * (na + ni), D.omega_inv, D.k, &D.n_inv, side);
    coeff_to_extended(d, D, polys, N * (na + ni), ext, side);
    const std::vector<G1> pts = commit_finish(d, pc);
    for (size_t p = 0; p < N; p++) {
      Proof& pr = proofs[p];
      for (size_t j = 0; j < na; j++) pr.tr.write_point(pts[p * na + j]);
      pr.theta = pr.tr.squeeze_challenge();
      pr.beta = pr.tr.squeeze_challenge();
      pr.gamma = pr.tr.squeeze_challenge();
    }
    trace.mark("advice committed");
  }

  Col values_of(size_t p, const ColRef& cr) const {
    if (cr.first == ADVICE) return column(advice_values, p * na + (size_t)cr.second, n);
    if (cr.first == FIXED) return column(K.fixed_values, (size_t)cr.second, n);
    return column(instance_values, p * ni + (size_t)cr.second, n);
  }

  // permutation grand products: rows [0, u = n - bf - 1] of every (proof, set)'s z column by one call whose scan walks a
  // proof's sets in order (key_shape cuts the columns into consecutive sets of deg - 2, the call's chunks, so set s of
  // proof p is column p nz + s of z_values); then the blinding rows, drawn proof by proof and set by set
  void permutation_products() {
    if (nz) {
      std::vector<const void*> values(N * np), sigma(np);
      std::vector<Fr> beta(N), gamma(N);
      for (size_t j = 0; j < np; j++) sigma[j] = column(K.sigma_values, j, n);
      for (size_t p = 0; p < N; p++) {
        for (size_t j = 0; j < np; j++) values[p * np + j] = values_of(p, K.circuit->permutation_columns[j]);
        beta[p] = proofs[p].beta;
        gamma[p] = proofs[p].gamma;
      }
      d.permutation_products(values, sigma, (size_t)(deg - 2), n - (uint32_t)bf - 1, beta, gamma, D.omega, delta, z_values, n);
      std::vector<Fr> blinds;
      for (size_t p = 0; p < N; p++)
        for (size_t si = 0; si < nz; si++) {
          for (int t = 0; t < bf; t++) blinds.push_back(items[p].rng.fr_random());
          (void)items[p].rng.fr_random();
        }
      Steps finish(*this);
      if (bf) finish.blinds(blinds, N * nz);
      finish.run();
    }
    trace.mark("grand products built");
  }

  // columns that one MSM launch may take with bases of their own: MSM_MAX_MULTI, and no more than one launch sequence of
  // this SRS's geometry holds (8 where the windows are wide enough for the two-level sort, from k = 18)
  size_t split_launch_columns() const {
    auto it = g_h2.bases.find(P.h_gl);
    if (it == g_h2.bases.end()) fail(H2_EHANDLE, "params bases released");
    return std::min<size_t>(MSM_MAX_MULTI, msm_cols_per_launch(it->second.geom, n));
  }

  // the vanishing argument's random polynomials (one ChaCha20 seed and n sequential draws each) and their commitments.
  // They come from the RNG, not from the transcript, so they are committed (over g) beside the permutation products
  // (over g_lagrange): one split launch while its columns fit split_launch_columns(), otherwise one launch per base; the
  // transcripts still receive the points in the reference's order
  void random_polys_and_commit() {
    for (size_t p = 0; p < N; p++) {
      uint8_t seed[32];
      items[p].rng.fill(seed, 32);
      uint32_t key[8];
      memcpy(key, seed, 32);
      hip_ok(d.ops->chacha20_scalars(column(random_polys, p, n), n, 0, key, d.s), "chacha20_scalars");
      (void)items[p].rng.fr_random();
    }
    const size_t mz = N * nz;
    std::vector<PendingCommit> pcs;
    if (mz + N <= split_launch_columns()) {
      pcs.push_back(commit_begin(d, P, z_values, n, mz + N, true, mz));
    } else {
      if (mz) pcs.push_back(commit_begin(d, P, z_values, n, mz, true));
      pcs.push_back(commit_begin(d, P, random_polys, n, N, false));
    }
    if (nz) {
      d.wait_msm_tail(side);                     // the z columns (blinding rows included) are final before that MSM
      Col zp = column(polys, N * (na + ni), n);
      hip_ok(hipMemcpyAsync(zp, z_values, mz * (size_t)n * 32, hipMemcpyDeviceToDevice, side), "hipMemcpyAsync(D2D)");
      d.ntt(zp, mz, D.omega_inv, D.k, &D.n_inv, side);
      coeff_to_extended(d, D, zp, mz, column(ext, N * (na + ni), en), side);
    }
    std::vector<G1> pts;
    for (auto& pc : pcs)
      for (auto& pt : commit_finish(d, pc)) pts.push_back(pt);
    for (size_t p = 0; p < N; p++) {
      for (size_t si = 0; si < nz; si++) proofs[p].tr.write_point(pts[p * nz + si]);
      proofs[p].tr.write_point(pts[mz + p]);
    }
    trace.mark("grand products + random polys committed");
  }

  // the quotients: one program, grid.y = proof, over every proof's extended columns
  void quotient() {
    advice_polys = polys;
    z_polys = column(polys, N * (na + ni), n);
    for (auto& pr : proofs) pr.y = pr.tr.squeeze_challenge();
    d.order(side, d.s, 2);                       // every coefficient and extended form is needed from here on
    Col h_ext = d.col(N * (size_t)en);
    {
      const ColumnMap& M = K.cmap;
      std::vector<const U128*> ptrs(N * (size_t)M.count);
      std::vector<uint32_t> masks(M.count, en - 1);
      masks[M.tinv] = (1u << (D.ext_k - D.k)) - 1;
      const size_t nc = K.prog.consts.size();
      std::vector<Fr> consts;
      for (size_t p = 0; p < N; p++) {
        const U128** t = ptrs.data() + p * (size_t)M.count;
        for (size_t j = 0; j < na; j++) t[M.advice0 + j] = column(ext, p * na + j, en);
        for (size_t j = 0; j < nf; j++) t[M.fixed0 + j] = column(K.fixed_ext, j, en);
        for (size_t j = 0; j < ni; j++) t[M.instance0 + j] = column(ext, N * na + p * ni + j, en);
        for (size_t j = 0; j < np; j++) t[M.sigma0 + j] = column(K.sigma_ext, j, en);
        for (size_t j = 0; j < nz; j++) t[M.z0 + j] = column(ext, N * (na + ni) + p * nz + j, en);
        t[M.l0] = K.basis_ext;
        t[M.l_last] = column(K.basis_ext, 1, en);
        t[M.l_blind] = column(K.basis_ext, 2, en);
        t[M.xcol] = K.xcol_ext;
        t[M.tinv] = K.tinv;
        std::vector<Fr> c = K.prog.consts;
        c[K.c_y] = proofs[p].y;
        c[K.c_beta] = proofs[p].beta;
        c[K.c_gamma] = proofs[p].gamma;
        for (size_t j = 0; j < np; j++) c[K.c_beta_delta[j]] = proofs[p].beta * delta.pow_u64((uint64_t)j);
        consts.insert(consts.end(), c.begin(), c.end());
      }
      expr_launch(d, K.prog, K.d_code, ptrs, masks, std::move(consts), nc, h_ext, en / n, en, N);
    }
    d.release(ext);
    // extended -> coefficients: inverse NTT with 1 / 2^ext_k, un-shift the coset, keep n (deg - 1) coefficients a proof
    const uint32_t hlen = n * (uint32_t)(deg - 1);
    h_pieces = d.col(N * (size_t)hlen);
    d.to_coeff(h_ext, D.ext_k, N, D.ext_omega_inv, D.en_inv, D.zeta_inv, h_pieces, hlen);
    d.release(h_ext);
    trace.mark("quotients enqueued");
    const std::vector<G1> pts = commit(d, P, h_pieces, n, N * (size_t)(deg - 1), false);
    for (size_t p = 0; p < N; p++) {
      for (int t = 0; t < deg - 1; t++) proofs[p].tr.write_point(pts[p * (size_t)(deg - 1) + t]);
      for (int t = 0; t < deg - 1; t++) (void)items[p].rng.fr_random();
    }
    trace.mark("quotients committed");
  }

  Col poly_of(size_t p, const Opening& o) const {
    switch (o.kind) {
      case POLY_ADVICE: return column(advice_polys, p * na + (size_t)o.index, n);
      case POLY_FIXED: return column(K.fixed_polys, (size_t)o.index, n);
      case POLY_SIGMA: return column(K.sigma_polys, (size_t)o.index, n);
      case POLY_Z: return column(z_polys, p * nz + (size_t)o.index, n);
      case POLY_RANDOM: return column(random_polys, p, n);
      default: return column(h_polys, p, n);
    }
  }

  // every proof's evaluations in one job list and one read-back
  void evaluate() {
    const OpeningPlan& L = K.plan;
    h_polys = d.col(N * (size_t)n);
    std::vector<std::pair<Col, Fr>> jobs;
    Lincombs hs;
    for (size_t p = 0; p < N; p++) {
      Proof& pr = proofs[p];
      pr.x = pr.tr.squeeze_challenge();
      for (auto& e : L.evals) jobs.push_back({poly_of(p, e), D.rotate(pr.x, e.rot)});
      if (L.shplonk) jobs.push_back({column(h_polys, p, n), pr.x});
      // h(X) = sum_i x^(n i) h_i(X)
      const Fr xn = pr.x.pow_u64(n);
      std::vector<std::pair<Col, Fr>> t;
      Fr pw = Fr::one();
      for (int i = 0; i < deg - 1; i++) {
        t.push_back({column(h_pieces, p * (size_t)(deg - 1) + i, n), pw});
        pw *= xn;
      }
      hs.add(column(h_polys, p, n), t);
    }
    Steps sums(*this);
    sums.lincomb(hs);
    sums.run();
    const std::vector<Fr> all = d.evaluate(jobs, n);
    const size_t per = jobs.size() / N;
    for (size_t p = 0; p < N; p++) {
      proofs[p].evals.assign(all.begin() + p * per, all.begin() + (p + 1) * per);
      for (size_t i = 0; i < L.evals.size(); i++) proofs[p].tr.write_scalar(proofs[p].evals[i]);
    }
    trace.mark("evaluations");
  }

  std::vector<Query> queries_of(size_t p) const {
    const OpeningPlan& L = K.plan;
    const Proof& pr = proofs[p];
    std::vector<Query> queries;
    for (auto& q : L.queries) {
      Fr value = Fr::zero();                     // h in a GWC proof: no value was computed, and that prover reads none
      if (q.eval >= 0) value = pr.evals[(size_t)q.eval];
      else if (L.shplonk) value = pr.evals.back();
      queries.push_back({D.rotate(pr.x, q.rot), poly_of(p, q), value});
    }
    return queries;
  }

  // ProverGWC::create_proof: one witness polynomial per distinct point, the v-power combination of everything opened
  // there.  Every (proof, point)'s combination in one launch, their synthetic divisions eight to a launch, one commit
  void gwc_open() {
    Lincombs accs_of;
    std::vector<Fr> points;                       // of all proofs, proof by proof
    std::vector<size_t> first(N + 1, 0);
    std::vector<std::vector<std::pair<Col, Fr>>> terms;
    for (size_t p = 0; p < N; p++) {
      const Fr v = proofs[p].tr.squeeze_challenge();
      const std::vector<Query> queries = queries_of(p);
      std::vector<Fr> mine;
      for (auto& q : queries)
        if (std::find(mine.begin(), mine.end(), q.point) == mine.end()) mine.push_back(q.point);
      for (auto& pt : mine) {
        std::vector<std::pair<Col, Fr>> t;
        Fr vp = Fr::one();
        for (auto& q : queries)
          if (q.point == pt) {
            t.push_back({q.poly, vp});
            vp *= v;
          }
        terms.push_back(std::move(t));
        points.push_back(pt);
      }
      first[p + 1] = points.size();
    }
    const size_t m = points.size();
    Col witnesses = d.col(m * (size_t)n), accs = d.col(m * (size_t)n);
    std::vector<Col> in, out;
    for (size_t q = 0; q < m; q++) {
      accs_of.add(column(accs, q, n), terms[q]);
      in.push_back(column(accs, q, n));
      out.push_back(column(witnesses, q, n));
    }
    Steps steps(*this);
    steps.lincomb(accs_of);
    steps.scan(in, out, points);
    steps.run();
    const std::vector<G1> pts = commit(d, P, witnesses, n, m, false);
    for (size_t p = 0; p < N; p++)
      for (size_t q = first[p]; q < first[p + 1]; q++) proofs[p].tr.write_point(pts[q]);
    trace.mark("openings committed");
  }

  // ProverSHPLONK::create_proof in its two halves around u: h of every proof behind one commit, then the final quotients
  // L(X) / (X - u) / z_0
  void shplonk_open() {
    std::vector<ShplonkOpening> O;
    for (size_t p = 0; p < N; p++) O.emplace_back(proofs[p].tr, queries_of(p));
    // the rotation sets are the plan's (a property of the key) unless two rotations of some x coincide: a proof with
    // fewer sets than the others sits out the steps of the sets it does not have
    size_t sets = 0;
    for (auto& o : O) sets = std::max(sets, o.groups.size());
    Col h = d.col(N * (size_t)n), acc = d.col(N * (size_t)n), quo = d.col(N * (size_t)n);
    std::vector<Col> src(N), dst(N);
    Steps first(*this);
    for (size_t gi = 0; gi < sets; gi++) {
      Lincombs sums;
      std::vector<Col> remainder_of;
      std::vector<std::vector<Fr>> rsums;
      size_t divisions = 0;
      for (size_t p = 0; p < N; p++) {
        if (gi >= O[p].groups.size()) continue;
        src[p] = column(acc, p, n);
        dst[p] = column(quo, p, n);
        sums.add(src[p], O[p].groups[gi].terms);
        remainder_of.push_back(src[p]);
        rsums.push_back(O[p].groups[gi].rsum);
        divisions = std::max(divisions, O[p].S.groups[gi].points.size());
      }
      first.lincomb(sums);
      first.sub_prefix(remainder_of, rsums);
      // divide by prod (X - point): one synthetic division per point, division t of every proof side by side,
      // ping-ponging two buffers (the quotient keeps the column's length, its top coefficients are zero)
      for (size_t t = 0; t < divisions; t++) {
        std::vector<Col> in, out;
        std::vector<Fr> z;
        for (size_t p = 0; p < N; p++) {
          if (gi >= O[p].groups.size() || t >= O[p].S.groups[gi].points.size()) continue;
          const auto& pts = O[p].S.groups[gi].points;
          in.push_back(src[p]);
          out.push_back(dst[p]);
          z.push_back(pts[t]);
          std::swap(src[p], dst[p]);
        }
        first.scan(in, out, z);
      }
      Lincombs into_h;
      for (size_t p = 0; p < N; p++) {
        if (gi >= O[p].groups.size()) continue;
        const Fr& vp = O[p].groups[gi].vp;
        Col hp = column(h, p, n);
        into_h.add(hp, gi == 0 ? std::vector<std::pair<Col, Fr>>{{src[p], vp}}
                               : std::vector<std::pair<Col, Fr>>{{hp, Fr::one()}, {src[p], vp}});
      }
      first.lincomb(into_h);
    }
    first.run();
    {
      const std::vector<G1> pts = commit(d, P, h, n, N, false);
      for (size_t p = 0; p < N; p++) proofs[p].tr.write_point(pts[p]);
    }
    Lincombs ls;
    std::vector<std::vector<Fr>> lconsts;
    std::vector<Col> accs, quos;
    std::vector<Fr> us;
    std::vector<pk::ScaleJob> scales;
    for (size_t p = 0; p < N; p++) {
      const Fr u = proofs[p].tr.squeeze_challenge();
      const ShplonkOpening::Final L = O[p].finish(u, column(h, p, n));
      accs.push_back(column(acc, p, n));
      quos.push_back(column(quo, p, n));
      ls.add(accs[p], L.terms);
      lconsts.push_back({L.lconst});
      us.push_back(u);
      scales.push_back({quos[p], L.z0_inv.v});
    }
    Steps second(*this);
    second.lincomb(ls);
    second.sub_prefix(accs, lconsts);
    second.scan(accs, quos, us);
    second.scale(scales);
    second.run();
    const std::vector<G1> pts = commit(d, P, quo, n, N, false);
    for (size_t p = 0; p < N; p++) proofs[p].tr.write_point(pts[p]);
    trace.mark("openings committed");
  }

  void run() {
    upload_instances_and_advice();
    commit_advice();
    permutation_products();
    random_polys_and_commit();
    quotient();
    evaluate();
    if (K.plan.shplonk) shplonk_open();
    else gwc_open();
  }
};

// proofs of `items`, in groups of at most g_prove_group; above k = 16, for which PROVE_GROUP is budgeted, the group halves
// with every doubling of the columns (down to one proof a group), so that the budget holds at every k
inline std::vector<std::vector<uint8_t>> create_proofs(ProvingKey& K, std::vector<Witness>& items, Trace& trace) {
  size_t per_group = g_prove_group;
  if (K.dom->k > PROVE_GROUP_K) per_group = std::max<size_t>(1, per_group >> (K.dom->k - PROVE_GROUP_K));
  std::vector<std::vector<uint8_t>> out;
  for (size_t g0 = 0; g0 < items.size(); g0 += per_group) {
    const size_t cnt = std::min(per_group, items.size() - g0);
    std::vector<Witness> group(std::make_move_iterator(items.begin() + g0), std::make_move_iterator(items.begin() + g0 + cnt));
    Proving B(K, group, trace);
    B.run();
    for (auto& pr : B.proofs) out.push_back(pr.tr.bytes());
  }
  return out;
}

}  // namespace product
}  // namespace h2
