// h2_keygen.hpp -- the evaluation domain, the proving key and its construction (keygen_vk + keygen_pk), the circuits of
// wasm.rs by index, and the keys kept between calls.
#pragma once
#include "h2_curve.hpp"
#include "h2_expr_program.hpp"
#include "h2_opening.hpp"

namespace h2 {
namespace product {

// ---- EvaluationDomain (halo2_proofs src/poly/domain.rs) ------------------------------------------------
struct Domain {
  uint32_t k, n, ext_k, en, qdeg;
  Fr omega, omega_inv, ext_omega, ext_omega_inv, zeta, zeta_inv, n_inv, en_inv;
  std::vector<Fr> t_evaluations;     // 1 / ((zeta w_ext^i)^n - 1), i < 2^(ext_k - k)
  Domain(uint32_t degree, uint32_t k_) : k(k_), n(1u << k_), qdeg(degree - 1) {
    ext_k = k;
    while ((1ull << ext_k) < (uint64_t)n * qdeg) ext_k++;
    if (ext_k > 28) fail(H2_EINVAL, "extended_k exceeds the field's two-adicity");
    en = 1u << ext_k;
    ext_omega = fr_root_of_unity();
    for (uint32_t i = ext_k; i < 28; i++) ext_omega = ext_omega.sqr();
    omega = ext_omega;
    for (uint32_t i = k; i < ext_k; i++) omega = omega.sqr();
    omega_inv = omega.inv();
    ext_omega_inv = ext_omega.inv();
    zeta = Fr::from_hex("0x30644e72e131a029048b6e193fd84104cc37a73fec2bc5e9b8ca0b2d36636f23");   // ZETA, as recalled (domain.py)
    zeta_inv = zeta.sqr();
    n_inv = Fr::from_u64(n).inv();
    en_inv = Fr::from_u64(en).inv();
    const uint32_t period = 1u << (ext_k - k);
    Fr cur = zeta;
    for (uint32_t i = 0; i < period; i++) {
      t_evaluations.push_back((cur.pow_u64(n) - Fr::one()).inv());
      cur *= ext_omega;
    }
  }
  Fr rotate(const Fr& x, int rot) const {
    const Fr w = rot >= 0 ? omega.pow_u64((uint64_t)rot) : omega_inv.pow_u64((uint64_t)(-rot));
    return x * w;
  }
};

// pseudo-columns of the program beyond the circuit's own: indices into the pointer table handed to the kernel
struct ColumnMap {
  int advice0, fixed0, instance0, sigma0, z0, l0, l_last, l_blind, xcol, tinv, count;
};

// what depends on the domain alone -- (k, constraint degree, blinding factors) -- and not on a circuit's columns or an
// SRS: w^i, the polynomial X and the three Lagrange-basis combinations l_0, l_last, l_blind on the extended coset,
// 1 / (X^n - 1).  Kept for the life of the process (a handful of shapes), shared by every key of that shape.
struct DomainKit {
  int device;
  uint32_t k, ext_k;
  int bf;
  std::unique_ptr<Dev> dev;
  Col omega_col = nullptr, xcol_ext = nullptr, basis_ext = nullptr, tinv = nullptr;
};
// shared with the keys built on a kit: the list below forgets its oldest entry, a key that still points into that kit's
// device buffers must keep them alive
inline std::vector<std::shared_ptr<DomainKit>> g_kits;

struct ProvingKey {
  std::unique_ptr<Circuit> circuit;
  std::unique_ptr<Domain> dom;
  const Params* params = nullptr;
  std::unique_ptr<Dev> dev;                 // owns the key's device buffers
  std::shared_ptr<const DomainKit> kit;     // owns omega_col, xcol_ext, basis_ext and tinv below
  int bf = 0;
  std::vector<std::vector<int>> sets;       // permutation columns, d - 2 per grand product
  Col fixed_values = nullptr, sigma_values = nullptr, fixed_polys = nullptr, sigma_polys = nullptr;
  Col fixed_ext = nullptr, sigma_ext = nullptr, basis_ext = nullptr /* l0, l_last, l_blind */, xcol_ext = nullptr;
  Col tinv = nullptr, omega_col = nullptr;
  std::vector<G1> fixed_commitments, sigma_commitments;
  Fr transcript_repr;
  ExprProgram prog;
  ColumnMap cmap{};
  int c_beta = -1, c_gamma = -1, c_y = -1;
  std::vector<int> c_beta_delta;            // beta * delta^j, one per permutation column
  const pk::XInstr* d_code = nullptr;
  OpeningPlan plan;                         // what a proof evaluates and opens, and where its compressed points sit
  size_t nf() const { return (size_t)circuit->num_fixed; }
  size_t np() const { return circuit->permutation_columns.size(); }
  // the key's transforms may still be running on the second stream when a key that is not kept dies (verify with
  // the key cache off): its blocks go back to the cache only once that stream is idle
  ~ProvingKey() {
    if (dev && dev->c->side_stream) (void)hipStreamSynchronize(dev->c->side_stream);
  }
};

inline Fr fr_delta() {   // DELTA = 7^(2^28): generator of the coset structure of the permutation argument
  Fr d = Fr::from_u64(7);
  for (int i = 0; i < 28; i++) d = d.sqr();
  return d;
}

// host group law on G1 (the same XYZZ templates as the kernels, host instantiation): a handful of operations per keygen
using HX = Xyzz<BN254_CURVE>;
inline HX hx_of(const G1& p) {
  if (p.inf) return HX::identity();
  return xyzz_from_affine(Affine<BN254_CURVE>{p.x.v, p.y.v});
}
inline std::vector<G1> hx_to_affine(const std::vector<HX>& pts) {       // one shared inversion
  std::vector<Fq> z(pts.size()), pre(pts.size());
  Fq acc = Fq::one();
  for (size_t j = 0; j < pts.size(); j++) {
    z[j] = Fq(pts[j].zzz);
    pre[j] = acc;
    if (!pts[j].is_identity()) acc *= z[j];
  }
  Fq inv = acc.inv();
  std::vector<G1> out(pts.size());
  for (size_t j = pts.size(); j-- > 0;) {
    if (pts[j].is_identity()) continue;
    const Fq zi3 = inv * pre[j];                                  // 1 / zzz
    inv *= z[j];
    const Fq zi = zi3 * Fq(pts[j].zz);                            // zz / zzz = 1 / z
    out[j].x = Fq(pts[j].x) * zi.sqr();
    out[j].y = Fq(pts[j].y) * zi3;
    out[j].inf = false;
  }
  return out;
}
inline HX hx_mul(const Fr& k, const HX& p) {
  uint8_t kb[32];
  k.to_le_bytes(kb);
  HX r = HX::identity();
  for (int i = 255; i >= 0; i--) {
    r = xyzz_double(r);
    if ((kb[i >> 3] >> (i & 7)) & 1) r = xyzz_add(r, p);
  }
  return r;
}

// coeff (m columns of n, stride n) -> extended-coset evaluations (m columns of en)
inline void coeff_to_extended(Dev& d, const Domain& D, Col in, size_t m, Col out, hipStream_t on = nullptr) {
  d.extend(in, D.n, D.k, m, D.zeta, D.ext_omega, D.ext_k, out, on);
}

inline std::shared_ptr<const DomainKit> domain_kit(const Domain& D, int bf, DevCtx* ctx) {
  for (auto& kp : g_kits)
    if (kp->device == ctx->device && kp->k == D.k && kp->ext_k == D.ext_k && kp->bf == bf) return kp;
  auto kit = std::make_shared<DomainKit>();
  kit->device = ctx->device;
  kit->k = D.k;
  kit->ext_k = D.ext_k;
  kit->bf = bf;
  kit->dev = std::make_unique<Dev>(ctx);
  Dev& d = *kit->dev;
  const uint32_t n = D.n;
  uint64_t w[4];
  // a ones column = the NTT of (1, 0, 0, ...) (every evaluation of the constant polynomial 1 is 1); then a[i] *= w^i
  kit->omega_col = d.col(n);
  {
    std::vector<SparseCol> c1(1);
    c1[0][0] = Fr::one();
    d.fill_sparse(kit->omega_col, n, c1);
    d.ntt(kit->omega_col, 1, D.omega, D.k);
    Dev::limbs(D.omega, w);
    hip_ok(d.ops->poly_powers(kit->omega_col, n, 1, w, d.s), "poly_powers");
  }
  // l_0, l_last, l_blind: Lagrange -> coefficients -> extended coset
  {
    Col basis = d.col(3 * (size_t)n);
    std::vector<SparseCol> b(3);
    b[0][0] = Fr::one();
    b[1][n - bf - 1] = Fr::one();
    for (uint32_t r = n - bf; r < n; r++) b[2][r] = Fr::one();
    d.fill_sparse(basis, n, b);
    d.ntt(basis, 3, D.omega_inv, D.k, &D.n_inv);
    kit->basis_ext = d.col(3 * (size_t)D.en);
    d.extend(basis, n, D.k, 3, D.zeta, D.ext_omega, D.ext_k, kit->basis_ext);
    d.release(basis);
  }
  // the polynomial X on the coset: zeta w_ext^i
  kit->xcol_ext = d.col(D.en);
  {
    std::vector<SparseCol> c1(1);
    c1[0][0] = D.zeta;
    d.fill_sparse(kit->xcol_ext, D.en, c1);
    d.ntt(kit->xcol_ext, 1, D.ext_omega, D.ext_k);                  // (zeta, zeta, ...)
    Dev::limbs(D.ext_omega, w);
    hip_ok(d.ops->poly_powers(kit->xcol_ext, D.en, 1, w, d.s), "poly_powers");
  }
  kit->tinv = d.upload_frs(D.t_evaluations);
  d.sync();
  if (g_kits.size() >= 8) g_kits.erase(g_kits.begin());
  g_kits.push_back(std::move(kit));
  return g_kits.back();
}

// ---- the circuits of wasm.rs by index ------------------------------------------------------------------------------------------
// a circuit, the index it stands for (any index other than 0 or 1 means Poseidon) and its multi-open scheme (wasm.rs:
// Collatz proves and verifies with SHPLONK, the other two with GWC); the entry points add the witness and the public inputs
struct Job {
  std::unique_ptr<Circuit> circuit;
  int index = 0;
  bool shplonk = false;
  std::vector<Fr> public_input;
};
inline Job make_circuit(int idx) {
  Job j;
  j.index = idx == 0 || idx == 1 ? idx : 2;
  j.shplonk = j.index == 0;
  if (j.index == 0) j.circuit = std::make_unique<CollatzCircuit>();
  else if (j.index == 1) j.circuit = std::make_unique<ArithmeticCircuit>();
  else j.circuit = std::make_unique<PoseidonCircuit>();
  return j;
}

// the permutation columns, d - 2 per grand product (halo2's chunking), and the blinding rows: host data of a key
inline void key_shape(ProvingKey& K) {
  const Circuit& C = *K.circuit;
  K.bf = C.blinding_factors();
  const int chunk = C.degree - 2;
  for (size_t s = 0; s < C.permutation_columns.size(); s += chunk) {
    std::vector<int> set;
    for (size_t j = s; j < std::min(s + chunk, C.permutation_columns.size()); j++) set.push_back((int)j);
    K.sets.push_back(set);
  }
}

// every gate, the permutation argument, the y-fold and the division by X^n - 1 as one program (host only)
inline void build_quotient_program(ProvingKey& K) {
  const Circuit& C = *K.circuit;
  const size_t np = K.np();
  ColumnMap& M = K.cmap;
  int next = 0;
  M.advice0 = next; next += C.num_advice;
  M.fixed0 = next; next += C.num_fixed;
  M.instance0 = next; next += C.num_instance;
  M.sigma0 = next; next += (int)np;
  M.z0 = next; next += (int)K.sets.size();
  M.l0 = next++; M.l_last = next++; M.l_blind = next++; M.xcol = next++; M.tinv = next++;
  M.count = next;
  ExprProgram& X = K.prog;
  std::function<int(const E&)> build = [&](const E& e) -> int {
    switch (e->kind) {
      case Expr::Const: return X.constant(e->c);
      case Expr::Advice: return X.column(M.advice0 + e->col, e->rot);
      case Expr::Fixed: return X.column(M.fixed0 + e->col, e->rot);
      case Expr::Instance: return X.column(M.instance0 + e->col, e->rot);
      case Expr::Neg: return X.sub(X.constant(Fr::zero()), build(e->a));
      case Expr::Sum:
        if (e->b->kind == Expr::Neg) return X.sub(build(e->a), build(e->b->a));
        return X.add(build(e->a), build(e->b));
      case Expr::Prod: return X.mul(build(e->a), build(e->b));
      case Expr::Scaled: return X.mul(build(e->a), X.constant(e->c));
    }
    return -1;
  };
  const int v_y = X.variable(&K.c_y), v_beta = X.variable(&K.c_beta), v_gamma = X.variable(&K.c_gamma);
  std::vector<int> v_bd(np);
  K.c_beta_delta.resize(np);
  for (size_t j = 0; j < np; j++) v_bd[j] = X.variable(&K.c_beta_delta[j]);
  const int one = X.constant(Fr::one());
  std::vector<int> terms;
  for (auto& g : C.gates) terms.push_back(build(g));
  auto colref = [&](const ColRef& cr) {
    return X.column((cr.first == ADVICE ? M.advice0 : cr.first == FIXED ? M.fixed0 : M.instance0) + cr.second, 0);
  };
  if (!K.sets.empty()) {
    const int l0 = X.column(M.l0, 0), l_last = X.column(M.l_last, 0), l_blind = X.column(M.l_blind, 0);
    const int nsets = (int)K.sets.size();
    auto z = [&](int i, int rot) { return X.column(M.z0 + i, rot); };
    terms.push_back(X.mul(l0, X.sub(one, z(0, 0))));
    terms.push_back(X.mul(l_last, X.sub(X.mul(z(nsets - 1, 0), z(nsets - 1, 0)), z(nsets - 1, 0))));
    for (int i = 1; i < nsets; i++) terms.push_back(X.mul(l0, X.sub(z(i, 0), z(i - 1, -(K.bf + 1)))));
    const int l_active = X.sub(X.sub(one, l_last), l_blind);
    const int xc = X.column(M.xcol, 0);
    for (int i = 0; i < nsets; i++) {
      int left = z(i, 1), right = z(i, 0);
      for (int j : K.sets[i]) {
        const int v = colref(C.permutation_columns[j]);
        left = X.mul(left, X.add(X.add(v, X.mul(X.column(M.sigma0 + j, 0), v_beta)), v_gamma));
        right = X.mul(right, X.add(X.add(v, X.mul(xc, v_bd[j])), v_gamma));
      }
      terms.push_back(X.mul(l_active, X.sub(left, right)));
    }
  }
  int numer = terms[0];
  for (size_t t = 1; t < terms.size(); t++) numer = X.add(X.mul(numer, v_y), terms[t]);
  const int root = X.mul(numer, X.column(M.tinv, 0));
  X.compile(root);
}

inline std::unique_ptr<ProvingKey> keygen(const Params& P, Job made, DevCtx* ctx) {
  Trace trace("keygen");
  auto pkp = std::make_unique<ProvingKey>();
  ProvingKey& K = *pkp;
  K.params = &P;
  K.circuit = std::move(made.circuit);
  const Circuit& C = *K.circuit;
  K.dom = std::make_unique<Domain>((uint32_t)C.degree, P.k);
  const Domain& D = *K.dom;
  K.dev = std::make_unique<Dev>(ctx);
  Dev& d = *K.dev;
  const uint32_t n = D.n;
  key_shape(K);
  K.plan = opening_plan(C, K.sets, K.bf, D.k, made.shplonk);
  if ((uint32_t)(K.bf + 1) >= n) fail(H2_EINVAL, "k too small for this circuit");
  const size_t nf = K.nf(), np = K.np();
  // fixed columns; the minimum rows a circuit needs are checked against n here
  std::vector<SparseCol> fixed = C.synthesize_fixed();
  for (auto& col : fixed)
    if (!col.empty() && col.rbegin()->first >= n - (uint32_t)(K.bf + 1)) fail(H2_EINVAL, "k too small for this circuit");
  Col lag = d.col((nf + np) * n);            // fixed then sigma, Lagrange form
  K.fixed_values = lag;
  K.sigma_values = lag + 2 * nf * (size_t)n;
  d.fill_sparse(K.fixed_values, n, fixed);
  // omega_col[i] = w^i (domain kit); sigma_j[i] = delta^j w^i except on the cells the copy constraints permute
  K.kit = domain_kit(D, K.bf, ctx);
  K.omega_col = K.kit->omega_col;
  K.basis_ext = K.kit->basis_ext;
  K.xcol_ext = K.kit->xcol_ext;
  K.tinv = K.kit->tinv;
  const Fr delta = fr_delta();
  std::vector<std::pair<std::pair<int, uint32_t>, Fr>> moved;     // (permutation column, row) -> its sigma value
  {
    std::vector<std::pair<Col, Fr>> t(1);
    Fr dj = Fr::one();
    for (size_t j = 0; j < np; j++) {
      t[0] = {K.omega_col, dj};
      d.lincomb(K.sigma_values + 2 * j * (size_t)n, n, t);
      dj *= delta;
    }
    auto mapping = permutation_mapping(C);
    std::vector<pk::CellRef> refs;
    std::vector<Fr> vals;
    for (auto& kv : mapping) {
      if (kv.first == kv.second) continue;
      if (kv.first.second >= n || kv.second.second >= n) fail(H2_EINVAL, "k too small for this circuit");
      refs.push_back({(uint32_t)kv.first.first, kv.first.second});
      vals.push_back(delta.pow_u64((uint64_t)kv.second.first) * D.omega.pow_u64(kv.second.second));
      moved.push_back({kv.first, vals.back()});
    }
    if (!refs.empty()) {
      const pk::CellRef* d_refs = (const pk::CellRef*)d.upload(refs.data(), refs.size() * sizeof(pk::CellRef));
      Col d_vals = d.upload_frs(vals);
      launch("scatter_cells_kernel", pk::scatter_cells_kernel, dim3((unsigned)((refs.size() + 255) / 256)), dim3(256), d.s,
             K.sigma_values, (size_t)n, d_refs, d_vals, (uint32_t)refs.size());
    }
  }
  // coefficient and extended forms of the fixed + sigma columns on the second stream, beside the commitment below and
  // the first phases of the proof (create_proof takes the second stream back before it needs them)
  Col polys = d.col((nf + np) * n);
  K.fixed_polys = polys;
  K.sigma_polys = polys + 2 * nf * (size_t)n;
  Col ext = d.col((nf + np) * (size_t)D.en);
  K.fixed_ext = ext;
  K.sigma_ext = ext + 2 * nf * (size_t)D.en;
  {
    hipStream_t side = d.side();
    d.order(d.s, side, 0);
    hip_ok(hipMemcpyAsync(polys, lag, (nf + np) * (size_t)n * 32, hipMemcpyDeviceToDevice, side), "hipMemcpyAsync(D2D)");
    d.ntt(polys, nf + np, D.omega_inv, D.k, &D.n_inv, side);
    coeff_to_extended(d, D, polys, nf + np, ext, side);
  }
  trace.mark("columns built");
  // commitments of the fixed + sigma columns, their coefficient and extended forms.  sigma_j = (identity permutation's
  // column j) + (the cells the copy constraints move): the first part's commitment is [delta^j] commit(w^i), kept
  // with the SRS; the second is sparse.  One MSM launch over nf + np SPARSE columns instead of np dense ones.
  if (P.sigma_identity.size() < np) {
    const G1 c_omega = commit(d, P, K.omega_col, n, 1, true)[0];
    std::vector<HX> pts;
    HX cur = hx_of(c_omega);
    for (size_t j = 0; j < std::max<size_t>(np, 8); j++) {
      pts.push_back(cur);
      cur = hx_mul(delta, cur);
    }
    P.sigma_identity = hx_to_affine(pts);
    trace.mark("identity permutation committed");
  }
  std::vector<G1> commits;
  {
    Col sparse = d.col((nf + np) * (size_t)n);
    d.copy(sparse, K.fixed_values, nf * (size_t)n * 32);
    std::vector<SparseCol> diff(np);
    for (auto& kv : moved) {
      const int j = kv.first.first;
      diff[j][kv.first.second] = kv.second - delta.pow_u64((uint64_t)j) * D.omega.pow_u64(kv.first.second);
    }
    d.fill_sparse(sparse + 2 * nf * (size_t)n, n, diff);
    commits = commit(d, P, sparse, n, nf + np, true);
    d.release(sparse);
    std::vector<HX> sums;
    for (size_t j = 0; j < np; j++) sums.push_back(xyzz_add(hx_of(P.sigma_identity[j]), hx_of(commits[nf + j])));
    const std::vector<G1> sig = hx_to_affine(sums);
    for (size_t j = 0; j < np; j++) commits[nf + j] = sig[j];
  }
  trace.mark("fixed + sigma committed");
  K.fixed_commitments.assign(commits.begin(), commits.begin() + nf);
  K.sigma_commitments.assign(commits.begin() + nf, commits.end());
  // vk digest
  const std::string s = vk_debug_string(C, D.k, D.ext_k, D.omega, K.fixed_commitments, K.sigma_commitments);
  K.transcript_repr = vk_transcript_repr(s);
  trace.mark("vk digest");

  build_quotient_program(K);
  ExprProgram& X = K.prog;
  K.d_code = (const pk::XInstr*)d.upload(X.code.data(), X.code.size() * sizeof(pk::XInstr));
  trace.mark("program compiled");     // no synchronisation here: create_proof queues behind keygen's kernels on the same
                                      // stream, and the staged host copies of the uploads live as long as the key
  if (trace.on) {
    size_t nmul = 0, ncol = 0;
    for (auto& ins : X.code) {
      if ((ins.op_dst >> 24) == 2) nmul++;
      if ((ins.a & (3u << 30)) == pk::X_COL) ncol++;
      if ((ins.b & (3u << 30)) == pk::X_COL) ncol++;
    }
    fprintf(stderr, "[h2 keygen] quotient program: %zu instructions (%zu products), %zu column reads, %u slots, %zu constants\n",
            X.code.size(), nmul, ncol, X.nslots, X.consts.size());
  }
  return pkp;
}

// proving keys kept between calls (the reference rebuilds them on every prove and verify, wasm.rs:86,95,114,132;
// a key depends only on the params and the circuit's fixed columns): keyed by params digest and circuit index
struct KeyEntry {
  std::array<uint8_t, 64> digest;
  int circuit;
  int device;                         // a key's columns live on one GPU
  std::unique_ptr<ProvingKey> key;
};
inline std::vector<KeyEntry> g_keys;
inline bool g_key_cache = true;

// the key for (params, circuit `slot` = a Job's index): cached or built now, from the EMPTY circuit; `owner` keeps a
// freshly built uncached key alive
inline ProvingKey& key_for(const Params& P, int slot, DevCtx* ctx, std::unique_ptr<ProvingKey>& owner) {
  if (g_key_cache) {
    for (auto& e : g_keys)
      if (e.circuit == slot && e.device == ctx->device && e.digest == P.digest) {
        e.key->params = &P;       // the params list may have been reordered since
        return *e.key;
      }
  }
  owner = keygen(P, make_circuit(slot), ctx);
  if (!g_key_cache) return *owner;
  if (g_keys.size() >= 6) g_keys.erase(g_keys.begin());
  g_keys.push_back({P.digest, slot, ctx->device, std::move(owner)});
  return *g_keys.back().key;
}

}  // namespace product
}  // namespace h2
