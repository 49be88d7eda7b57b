// h2_product_dev.hpp -- the device plumbing of the product surface: columns in HBM and the block cache behind them (Dev),
// the SRS (Params), the commit phases (one MSM launch sequence each, spread over the contexts when there are several)
// and the table-free small MSM of the verifiers.
#pragma once
#include <algorithm>
#include <array>
#include <thread>

#include "h2_circuits.hpp"
#include "h2_expr_program.hpp"
#include "h2_pairing.hpp"
#include "h2_poly.hpp"
#include "h2_product_base.hpp"
#include "h2_prover_kernels.hpp"

namespace h2 {
namespace product {
using namespace h2::plonk;

// ---- device side plumbing ---------------------------------------------------------------------------------------------
using Col = U128*;    // a column of field elements in HBM (n or 2^extended_k of them)

struct Dev {
  DevCtx* c;
  hipStream_t s;
  const CurveOps* ops;
  std::vector<std::pair<void*, size_t>> live;                 // everything handed out, freed by the owner's destructor
  std::vector<std::vector<uint8_t>> staged;                   // host buffers of in-flight uploads (kept until sync)
  // cache of freed blocks keyed by (device, size): hipMalloc / hipFree synchronise the device, a proof needs ~60 buffers
  using BlockKey = std::pair<int, size_t>;
  static std::multimap<BlockKey, void*>& cache() {
    static auto* m = new std::multimap<BlockKey, void*>();   // never destroyed: keys cached until process exit release into it
    return *m;
  }
  explicit Dev(DevCtx* ctx) : c(ctx), s(ctx->stream), ops(ops_of(H2_BN254)) {}
  void* alloc(size_t bytes) {
    bytes = (bytes + 255) & ~(size_t)255;
    void* p = nullptr;
    auto it = cache().find(BlockKey{c->device, bytes});
    if (it != cache().end()) {
      p = it->second;
      cache().erase(it);
    } else if (int rc = device_alloc(&p, bytes, "block"); rc != H2_OK) {
      fail(rc, g_h2.last_error);
    }
    live.push_back({p, bytes});
    return p;
  }
  Col col(size_t elems) { return (Col)alloc(elems * 32); }
  // give everything back to the cache (the stream is in order: a later user of the block queues behind this one)
  void release_all() {
    for (auto& b : live) cache().insert({BlockKey{c->device, b.second}, b.first});
    live.clear();
  }
  void release(void* p) {
    for (size_t i = 0; i < live.size(); i++)
      if (live[i].first == p) {
        cache().insert({BlockKey{c->device, live[i].second}, p});
        live.erase(live.begin() + i);
        return;
      }
  }
  void sync() {
    hip_ok(hipStreamSynchronize(s), "hipStreamSynchronize");
    staged.clear();
  }
  void* upload(const void* data, size_t bytes) {
    staged.emplace_back((const uint8_t*)data, (const uint8_t*)data + bytes);
    void* d = alloc(bytes);
    hip_ok(hipMemcpyAsync(d, staged.back().data(), bytes, hipMemcpyHostToDevice, s), "hipMemcpyAsync(H2D)");
    return d;
  }
  Col upload_frs(const std::vector<Fr>& v) {
    std::vector<uint8_t> raw(v.size() * 32);
    for (size_t i = 0; i < v.size(); i++) memcpy(raw.data() + 32 * i, v[i].v.v, 32);
    return (Col)upload(raw.data(), raw.size());
  }
  std::vector<Fr> download_frs(const void* d, size_t count) {
    std::vector<uint8_t> raw(count * 32);
    hip_ok(hipMemcpyAsync(raw.data(), d, raw.size(), hipMemcpyDeviceToHost, s), "hipMemcpyAsync(D2H)");
    sync();
    std::vector<Fr> out(count);
    for (size_t i = 0; i < count; i++) out[i] = Fr::from_mont_limbs(raw.data() + 32 * i);
    return out;
  }
  void zero(void* p, size_t bytes) { hip_ok(hipMemsetAsync(p, 0, bytes, s), "hipMemsetAsync"); }
  void copy(void* dst, const void* src, size_t bytes) {
    hip_ok(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, s), "hipMemcpyAsync(D2D)");
  }
  static void limbs(const Fr& f, uint64_t out[4]) { f.mont_limbs(out); }
  // m sparse columns -> m dense device columns (stride `stride` elements), zero elsewhere
  void fill_sparse(Col base, size_t stride, const std::vector<SparseCol>& cols) {
    zero(base, cols.size() * stride * 32);
    std::vector<pk::CellRef> refs;
    std::vector<Fr> vals;
    for (size_t j = 0; j < cols.size(); j++)
      for (auto& kv : cols[j]) {
        refs.push_back({(uint32_t)j, kv.first});
        vals.push_back(kv.second);
      }
    if (refs.empty()) return;
    const pk::CellRef* d_refs = (const pk::CellRef*)upload(refs.data(), refs.size() * sizeof(pk::CellRef));
    Col d_vals = upload_frs(vals);
    launch("scatter_cells_kernel", pk::scatter_cells_kernel, dim3((unsigned)((refs.size() + 255) / 256)), dim3(256), s, base,
           stride, d_refs, d_vals, (uint32_t)refs.size());
  }
  void ntt(Col a, size_t m, const Fr& omega, uint32_t log_n, const Fr* scale = nullptr, hipStream_t on = nullptr) {
    uint64_t w[4], sc[4];
    limbs(omega, w);
    if (scale) limbs(*scale, sc);
    st_ok(ntt_enqueue(*c, H2_BN254, a, m, w, log_n, on ? on : s, scale ? sc : nullptr), "ntt_enqueue");
  }
  // m columns of 2^log_n coefficients (stride `stride` elements) -> their 2^ext_log_n values on the coset zeta <ext_omega>
  // in `out` (another buffer): one call, the zero padding never written or read (h2_ntt29.hpp's extending pass 0)
  void extend(Col in, size_t stride, uint32_t log_n, size_t m, const Fr& zeta, const Fr& ext_omega, uint32_t ext_log_n, Col out,
              hipStream_t on = nullptr) {
    uint64_t z[4], w[4];
    limbs(zeta, z);
    limbs(ext_omega, w);
    st_ok(coeff_to_extended_enqueue(*c, H2_BN254, in, stride, log_n, m, z, w, ext_log_n, out, on ? on : s),
          "coeff_to_extended_enqueue");
  }
  // `on` waits for the accumulate kernel of the MSM enqueued last on this context (commit_begin)
  void wait_msm_tail(hipStream_t on) {
    if (c->tail_recorded && c->tail_wait) hip_ok(hipStreamWaitEvent(on, c->tail_wait, 0), "hipStreamWaitEvent(tail)");
  }
  // the second stream of this context (non-blocking) and three events to hand work back and forth
  hipStream_t side() {
    if (!c->side_stream) {
      hip_ok(hipStreamCreateWithFlags(&c->side_stream, hipStreamNonBlocking), "hipStreamCreateWithFlags");
      for (auto& e : c->side_ev) hip_ok(hipEventCreateWithFlags(&e, hipEventDisableTiming), "hipEventCreateWithFlags");
    }
    return c->side_stream;
  }
  // `to` waits for everything enqueued on `from` so far
  void order(hipStream_t from, hipStream_t to, int ev) {
    side();
    hip_ok(hipEventRecord(c->side_ev[ev], from), "hipEventRecord");
    hip_ok(hipStreamWaitEvent(to, c->side_ev[ev], 0), "hipStreamWaitEvent");
  }
  void lincomb(Col out, uint32_t n, const std::vector<std::pair<Col, Fr>>& terms) {
    bool accumulate = false;
    for (size_t lo = 0; lo < terms.size(); lo += pk::LINCOMB_MAX) {
      pk::LincombArgs A{};
      A.count = (int)std::min<size_t>(pk::LINCOMB_MAX, terms.size() - lo);
      for (int j = 0; j < A.count; j++) {
        A.a[j] = terms[lo + j].first;
        A.c[j] = terms[lo + j].second.v;
      }
      A.unit_first = terms[lo].second == Fr::one();
      launch("lincomb_kernel", pk::lincomb_kernel, dim3((n + 255) / 256), dim3(256), s, A, out, n, accumulate ? 1 : 0);
      accumulate = true;
    }
  }
  // q_j = (a_j - a_j(z_j)) / (X - z_j) -- all jobs in one launch sequence
  void scan_batch(uint32_t n, const std::vector<Col>& in, const std::vector<Col>& out, const std::vector<Fr>& z) {
    for (size_t j0 = 0; j0 < in.size(); j0 += SCAN_MAX_JOBS) {
      const size_t cnt = std::min<size_t>(SCAN_MAX_JOBS, in.size() - j0);
      const void* a[SCAN_MAX_JOBS];
      void* o[SCAN_MAX_JOBS];
      uint64_t zl[SCAN_MAX_JOBS][4];
      for (size_t j = 0; j < cnt; j++) {
        a[j] = in[j0 + j];
        o[j] = out[j0 + j];
        limbs(z[j0 + j], zl[j]);
      }
      void* ws = alloc(cnt * SCAN_WS_BYTES);
      hip_ok(ops->poly_scan(0, a, o, zl[0], (uint32_t)cnt, n, ws, s), "poly_scan");
      release(ws);
    }
  }
  // values of `jobs` = (polynomial, point) pairs, all polynomials of n coefficients: one job table, one read-back
  std::vector<Fr> evaluate(const std::vector<std::pair<Col, Fr>>& jobs, uint32_t n) {
    if (jobs.empty()) return {};
    std::vector<const void*> polys(jobs.size());
    std::vector<uint64_t> points(4 * jobs.size());
    for (size_t i = 0; i < jobs.size(); i++) {
      polys[i] = jobs[i].first;
      limbs(jobs[i].second, points.data() + 4 * i);
    }
    Col out = col(jobs.size());
    st_ok(poly_eval_enqueue(*c, H2_BN254, polys.data(), n, points.data(), jobs.size(), out, s), "poly_eval_enqueue");
    std::vector<Fr> v = download_frs(out, jobs.size());
    release(out);
    return v;
  }
  // m extended columns (2^ext_log_n values on the coset zeta <ext_omega>, read only) -> the first out_len coefficients of
  // each, contiguous in `out`: the inverse transform scaled by `scale`, the coset shift undone and the cut in one call
  void to_coeff(Col ext, uint32_t ext_log_n, size_t m, const Fr& ext_omega_inv, const Fr& scale, const Fr& zeta_inv, Col out,
                size_t out_len) {
    uint64_t w[4], sc[4], zi[4];
    limbs(ext_omega_inv, w);
    limbs(scale, sc);
    limbs(zeta_inv, zi);
    st_ok(extended_to_coeff_enqueue(*c, H2_BN254, ext, ext_log_n, m, w, sc, zi, nullptr, 0, out, out_len, out_len, s),
          "extended_to_coeff_enqueue");
  }
  // the permutation argument's grand products of m proofs (h2_permutation.hpp): proof p's n_cols columns at
  // values[p n_cols ...], cut into sets of chunk_len; rows [0, u] of its sets' z columns at z + (p S + set) n, chained on the
  // device
  void permutation_products(const std::vector<const void*>& values, const std::vector<const void*>& sigma, size_t chunk_len, uint32_t u,
                            const std::vector<Fr>& beta, const std::vector<Fr>& gamma, const Fr& omega, const Fr& delta, Col z,
                            uint32_t n) {
    const size_t m = beta.size();
    std::vector<uint64_t> b(4 * m), g(4 * m);
    for (size_t p = 0; p < m; p++) {
      limbs(beta[p], b.data() + 4 * p);
      limbs(gamma[p], g.data() + 4 * p);
    }
    uint64_t w[4], dl[4];
    limbs(omega, w);
    limbs(delta, dl);
    st_ok(permutation_product_enqueue(*c, H2_BN254, values.data(), sigma.data(), sigma.size(), chunk_len, u, m, b.data(), g.data(), w, dl,
                                      z, n, s),
          "permutation_product_enqueue");
  }
  ~Dev() { release_all(); }
};

// expr_kernel over en rows of `count` proofs (grid.y = proof): one program and one set of row masks; proof p's column
// pointers at ptrs[p masks.size() ...], its constants (c, patched for the proof) at consts[p nconsts ...], uploaded in the
// kernel's working form c 2^261, its result at out + p en; the LDS of the slots beyond the registers is checked against
// what one workgroup may hold before anything is uploaded or launched.  create_proofs and the test hook
// h2_selftest_expr_run (count = 1) both launch the quotient program through here, the kernel's bn256::Fr instantiation
// through the curve's launch table as h2_expr_eval_device launches it.
inline void expr_launch(Dev& d, const ExprProgram& X, const pk::XInstr* d_code, const std::vector<const U128*>& ptrs,
                        const std::vector<uint32_t>& masks, std::vector<Fr> consts, size_t nconsts, Col out, uint32_t step,
                        uint32_t en, size_t count) {
  const size_t lds = expr_lds_bytes(X);
  if (ptrs.size() != count * masks.size() || consts.size() != count * nconsts) fail(H2_EINVAL, "expr_launch: table sizes");
  const void* const* d_ptrs = (const void* const*)d.upload(ptrs.data(), ptrs.size() * sizeof(void*));
  const uint32_t* d_masks = (const uint32_t*)d.upload(masks.data(), masks.size() * 4);
  for (auto& c : consts)
    for (int t = 0; t < 5; t++) c = c + c;            // c 2^256 -> c 2^261: the kernel's working form (R' = 2^261)
  Col d_consts = d.upload_frs(consts);
  hip_ok(d.ops->expr_launch(d_code, (uint32_t)X.code.size(), d_ptrs, (uint32_t)masks.size(), d_masks, d_consts, (uint32_t)nconsts, out,
                            en, step, en, (uint32_t)count, lds, d.s),
         "expr_kernel");
}

// the context an entry point works on
inline DevCtx* the_ctx() {
  if (!g_h2.ready) fail(H2_ENOTINIT, "h2_init has not been called");
  DevCtx* c = ctx_current();
  if (!c) fail(H2_EINVAL, "no h2 context on the current HIP device");
  return c;
}

// ---- params: the SRS registered once per distinct byte string -----------------------------------------------------------
struct Params {
  uint32_t k = 0;
  uint64_t h_g = 0, h_gl = 0;       // bases handles (g, g_lagrange)
  G1 g0;
  bn::G2 g2, s_g2;
  std::array<uint8_t, 64> digest{};
  // [delta^j] commit_lagrange(w^i): the commitment of the IDENTITY permutation's column j -- a property of the SRS, not
  // of a circuit.  A circuit's sigma_j differs from it in the few cells its copy constraints move, so its
  // commitment is this point plus a sparse MSM (keygen would otherwise commit to 7 dense columns on every call)
  mutable std::vector<G1> sigma_identity;
};
inline std::vector<Params> g_params;       // small LRU: the UI keeps one SRS, tests a few

inline Fq fq_from_mont(const uint8_t* p) { return Fq::from_mont_limbs(p); }

inline G1 affine_from_raw(const uint8_t* p) {
  G1 g;
  g.x = fq_from_mont(p);
  g.y = fq_from_mont(p + 32);
  g.inf = g.x.is_zero() && g.y.is_zero();
  return g;
}

inline const Params& params_get(const uint8_t* bytes, size_t len) {
  if (!bytes || len < 4) fail(H2_EPROOF, "params: truncated");
  uint32_t k;
  memcpy(&k, bytes, 4);
  if (k > 28) fail(H2_EPROOF, "params: k out of range");
  const size_t n = (size_t)1 << k;
  if (len != 4 + 128 * n + 256) fail(H2_EPROOF, "params: wrong length for k");
  // cache key: multiply-xorshift lanes over every byte (eight interleaved lanes keep one core's multiplier busy:
  // 17 GB/s, 0.48 ms of every call at k = 16; Blake2b took 8 ms), the blob cut into four quarters hashed by four threads
  // (0.48 -> ~0.15 ms), finished through Blake2b -- a fingerprint against accidents, not against a caller attacking
  // itself (include/h2hip.h, "Trust")
  constexpr int PARTS = 4;
  uint64_t lane[PARTS][8];
  auto hash_part = [&](int part) {
    static const uint64_t seed[8] = {0x9E3779B97F4A7C15ull, 0xBF58476D1CE4E5B9ull, 0x94D049BB133111EBull, 0xD6E8FEB86659FD93ull,
                                     0xA0761D6478BD642Full, 0xE7037ED1A0B428DBull, 0x8EBC6AF09C88C6E3ull, 0x589965CC75374CC3ull};
    uint64_t* l = lane[part];
    for (int i = 0; i < 8; i++) l[i] = seed[i] + (uint64_t)part;
    const size_t blocks = len / 64, per = (blocks + PARTS - 1) / PARTS;
    const size_t b0 = std::min(blocks, per * part), b1 = std::min(blocks, b0 + per);
    const uint8_t* q = bytes + 64 * b0;
    for (size_t i = b0; i < b1; i++, q += 64) {
      uint64_t w[8];
      memcpy(w, q, 64);
      for (int k = 0; k < 8; k++) {
        l[k] = (l[k] ^ w[k]) * 0xFF51AFD7ED558CCDull;
        l[k] ^= l[k] >> 29;
      }
    }
    if (part == PARTS - 1)
      for (q = bytes + 64 * blocks; q < bytes + len; q++) l[0] = (l[0] ^ *q) * 0x100000001B3ull;
  };
  std::thread th[PARTS - 1];
  for (int t = 1; t < PARTS; t++) {
    try {
      if (len >= (1u << 20)) th[t - 1] = std::thread(hash_part, t);
      else hash_part(t);
    } catch (const std::exception&) {   // no thread to be had: the part is hashed here, into its own lanes all the same
      hash_part(t);
    }
  }
  hash_part(0);
  for (auto& t : th)
    if (t.joinable()) t.join();
  Blake2b h;
  h.update(lane, sizeof lane);
  h.update(&len, sizeof len);
  h.update(bytes, 4);
  h.update(bytes + len - 256, 256);
  std::array<uint8_t, 64> dg;
  h.digest(dg.data());
  for (size_t i = 0; i < g_params.size(); i++)
    if (g_params[i].digest == dg) {
      if (i) std::swap(g_params[i], g_params[0]);
      return g_params[0];
    }
  Params p;
  p.k = k;
  p.digest = dg;
  // the reference reads with SerdeFormat::RawBytes (wasm.rs:79-80): raw Montgomery limbs, 64 B per G1 point
  int rc = h2_bases_register(H2_BN254, (const uint64_t*)(bytes + 4), n, &p.h_g);
  if (rc == H2_EINVAL) fail(H2_EPROOF, "params: g holds a point that is not on the curve");
  st_ok(rc, "h2_bases_register(g)");
  rc = h2_bases_register(H2_BN254, (const uint64_t*)(bytes + 4 + 64 * n), n, &p.h_gl);
  if (rc != H2_OK) (void)h2_bases_release(p.h_g);
  if (rc == H2_EINVAL) fail(H2_EPROOF, "params: g_lagrange holds a point that is not on the curve");
  st_ok(rc, "h2_bases_register(g_lagrange)");
  p.g0 = affine_from_raw(bytes + 4);
  const uint8_t* t = bytes + 4 + 128 * n;
  p.g2 = bn::G2{{fq_from_mont(t), fq_from_mont(t + 32)}, {fq_from_mont(t + 64), fq_from_mont(t + 96)}, false};
  p.s_g2 = bn::G2{{fq_from_mont(t + 128), fq_from_mont(t + 160)}, {fq_from_mont(t + 192), fq_from_mont(t + 224)}, false};
  if (g_params.size() >= 4) {
    (void)h2_bases_release(g_params.back().h_g);
    (void)h2_bases_release(g_params.back().h_gl);
    g_params.pop_back();
  }
  g_params.insert(g_params.begin(), p);
  return g_params[0];
}

// [k] pt on the twist (affine, host): the [s]G2 of ParamsKZG::new
inline bn::G2 g2_mul(const Fr& k, const bn::G2& pt) {
  uint8_t kb[32];
  k.to_le_bytes(kb);
  bn::G2 r;   // identity
  auto add = [](const bn::G2& a, const bn::G2& b) {
    if (a.inf) return b;
    if (b.inf) return a;
    bn::F2 lam;
    if (a.x == b.x) {
      if (!(a.y == b.y) || a.y.is_zero()) return bn::G2{};
      lam = bn::scale(bn::sqr(a.x), Fq::from_u64(3)) * bn::inv(bn::scale(a.y, Fq::from_u64(2)));
    } else {
      lam = (b.y - a.y) * bn::inv(b.x - a.x);
    }
    bn::G2 o;
    o.x = bn::sqr(lam) - a.x - b.x;
    o.y = lam * (a.x - o.x) - a.y;
    o.inf = false;
    return o;
  };
  for (int i = 255; i >= 0; i--) {
    r = add(r, r);
    if ((kb[i >> 3] >> (i & 7)) & 1) r = add(r, pt);
  }
  return r;
}

// Jacobian -> affine on the host: m inversions folded into one (a one-thread device kernel took 0.35 ms per phase)
inline std::vector<G1> jacobian_to_affine_host(const std::vector<uint8_t>& raw, size_t m) {
  std::vector<Fq> zs(m), pre(m);
  Fq acc = Fq::one();
  for (size_t j = 0; j < m; j++) {
    zs[j] = Fq::from_mont_limbs(raw.data() + 96 * j + 64);
    pre[j] = acc;
    if (!zs[j].is_zero()) acc *= zs[j];
  }
  Fq inv = acc.inv();
  std::vector<G1> pts(m);
  for (size_t j = m; j-- > 0;) {
    if (zs[j].is_zero()) continue;                     // identity
    const Fq zi = inv * pre[j], zi2 = zi.sqr();
    inv *= zs[j];
    pts[j].x = Fq::from_mont_limbs(raw.data() + 96 * j) * zi2;
    pts[j].y = Fq::from_mont_limbs(raw.data() + 96 * j + 32) * zi2 * zi;
    pts[j].inf = false;
  }
  return pts;
}

// The MSM of a commit phase is enqueued by commit_begin and read back by commit_finish: what is queued between the two
// on the second stream behind Dev::wait_msm_tail starts when the accumulate kernel of that MSM has finished, i.e. runs
// beside the MSM's small-grid tail instead of competing with its sort and accumulate kernels (started at once, the
// advice transforms made the sort kernels of the advice commitment three times slower: 140 against 48 us).
struct PendingCommit {
  void* out = nullptr;
  size_t m = 0;
};
// With several contexts (h2_init_devices) a commit phase is spread over them by POINT RANGE (SURVEY.md section 8(e),
// as sharded.msm_phase_device does across ranks): context g commits rows / bases [n g / G, n (g+1) / G) of EVERY column
// of the phase against its own replica of the table, so phases of m = 1 .. 5 columns use every GPU.  The other
// contexts' shares of the columns travel device to device (peer copies, cnt * 32 bytes per column), their G x m partial
// sums (96 bytes each) come back the same way and are added on the prover's device (points_sum_kernel): the same group
// elements as the one-device commitment, hence the same proof bytes.  Transforms are NOT spread: a column would cross
// xGMI twice (2 x 16 MiB for an extended column at k = 16, ~0.5 ms) for ~60 us of butterflies.
inline uint64_t g_sharded_commits = 0;
inline uint64_t g_commit_launches = 0;            // commit_begin calls since the library was loaded (tests)
inline size_t g_shard_min_rows = 1024;            // per context; below this the copies and the extra launches cost more than they save
// `split` < m: columns [0, split) commit against g_lagrange and [split, m) against g IN THE SAME LAUNCH (commitments
// that do not wait for each other: the permutation products and the RNG-drawn random polynomial)
inline PendingCommit commit_begin(Dev& d, const Params& P, Col cols, uint32_t n, size_t m, bool lagrange, size_t split = ~(size_t)0) {
  auto it = g_h2.bases.find(lagrange ? P.h_gl : P.h_g);
  if (it == g_h2.bases.end()) fail(H2_EHANDLE, "params bases released");
  g_commit_launches++;
  PendingCommit pc;
  pc.m = m;
  pc.out = d.alloc(m * 96);
  d.c->tail_wanted = true;                   // the MSM records an event behind its accumulate kernel (Dev::wait_msm_tail)
  std::vector<const BasesEntry*> per;
  const BasesEntry* be = &it->second;
  if (split < m) {
    auto ig = g_h2.bases.find(P.h_g), il = g_h2.bases.find(P.h_gl);
    if (ig == g_h2.bases.end() || il == g_h2.bases.end()) fail(H2_EHANDLE, "params bases released");
    per.resize(m);
    for (size_t j = 0; j < m; j++) per[j] = j < split ? &il->second : &ig->second;
    be = &il->second;
  }
  const BasesEntry* const* perp = per.empty() ? nullptr : per.data();
  const size_t G = g_h2.ctx.size();
  if (G == 1 || (size_t)n < g_shard_min_rows * G) {
    st_ok(msm_device_run(*d.c, H2_BN254, *be, cols, 0, n, n, m, pc.out, false, d.s, perp), "msm_device_run");
    return pc;
  }
  g_sharded_commits++;
  const size_t self = ctx_index(d.c);
  char* partials = (char*)d.alloc(G * m * 96);
  auto event_of = [](DevCtx& c) {
    if (!c.shard_ev) hip_ok(hipEventCreateWithFlags(&c.shard_ev, hipEventDisableTiming), "hipEventCreateWithFlags");
    return c.shard_ev;
  };
  hip_ok(hipEventRecord(event_of(*d.c), d.s), "hipEventRecord");            // the columns are final from here on
  size_t slot = 1;
  for (size_t g = 0; g < G; g++) {
    if (g == self) continue;
    DevCtx& cg = g_h2.ctx[g];
    DeviceGuard dg(cg.device);
    const size_t lo = (size_t)n * slot / G, hi = (size_t)n * (slot + 1) / G, cnt = hi - lo;
    const size_t res_off = (m * cnt * 32 + 255) & ~(size_t)255;
    ArenaLease stage(cg.stage, res_off + m * 96, cg.stream);
    st_ok(stage.rc, "arena");
    hip_ok(hipStreamWaitEvent(cg.stream, d.c->shard_ev, 0), "hipStreamWaitEvent");
    for (size_t j = 0; j < m; j++)
      hip_ok(hipMemcpyPeerAsync((char*)cg.stage.p + j * cnt * 32, cg.device, (const char*)cols + (j * (size_t)n + lo) * 32,
                                d.c->device, cnt * 32, cg.stream), "hipMemcpyPeerAsync(columns)");
    void* d_res = (char*)cg.stage.p + res_off;
    st_ok(msm_device_run(cg, H2_BN254, *be, cg.stage.p, lo, cnt, cnt, m, d_res, false, cg.stream, perp), "msm_device_run");
    hip_ok(hipMemcpyPeerAsync(partials + slot * m * 96, d.c->device, d_res, cg.device, m * 96, cg.stream),
           "hipMemcpyPeerAsync(partials)");
    hip_ok(hipEventRecord(event_of(cg), cg.stream), "hipEventRecord");
    st_ok(stage.release(), "arena");
    slot++;
  }
  // this context's share: rows [0, n / G)
  st_ok(msm_device_run(*d.c, H2_BN254, *be, cols, 0, (size_t)n / G, n, m, partials, false, d.s, perp), "msm_device_run");
  for (size_t g = 0; g < G; g++)
    if (g != self) hip_ok(hipStreamWaitEvent(d.s, g_h2.ctx[g].shard_ev, 0), "hipStreamWaitEvent");
  hip_ok(d.ops->points_sum(partials, pc.out, (uint32_t)G, (uint32_t)m, d.s), "points_sum");
  d.release(partials);
  return pc;
}
inline std::vector<G1> commit_finish(Dev& d, PendingCommit& pc) {
  std::vector<uint8_t> raw(pc.m * 96);
  hip_ok(hipMemcpyAsync(raw.data(), pc.out, raw.size(), hipMemcpyDeviceToHost, d.s), "hipMemcpyAsync(D2H)");
  d.sync();
  d.release(pc.out);
  pc.out = nullptr;
  return jacobian_to_affine_host(raw, pc.m);
}
// m columns of n scalars -> m commitments (affine, canonical coordinates)
inline std::vector<G1> commit(Dev& d, const Params& P, Col cols, uint32_t n, size_t m, bool lagrange, size_t split = ~(size_t)0) {
  PendingCommit pc = commit_begin(d, P, cols, n, m, lagrange, split);
  return commit_finish(d, pc);
}

// up to four lists of terms (64-byte points and 32-byte scalars in the API form; no identities, no zero scalars) -> their
// sums, in ONE launch of the table-free small MSM (msm_small_kernel: one quad per term); an empty list gives the identity
inline std::vector<G1> msm_small_run(Dev& d, const std::vector<std::vector<uint8_t>>& pts, const std::vector<std::vector<uint8_t>>& sc) {
  const size_t count = pts.size();
  std::vector<G1> out(count);
  std::vector<const void*> d_pts, d_sc;
  std::vector<uint32_t> ms, live;
  size_t mmax = 0;
  for (size_t j = 0; j < count; j++) {
    const size_t m = pts[j].size() / 64;
    if (m == 0) continue;
    d_pts.push_back(d.upload(pts[j].data(), pts[j].size()));
    d_sc.push_back(d.upload(sc[j].data(), sc[j].size()));
    ms.push_back((uint32_t)m);
    live.push_back((uint32_t)j);
    mmax = std::max(mmax, m);
  }
  if (live.empty()) return out;
  const size_t blocks = (mmax + 15) / 16, nl = live.size();
  Col work = d.col((nl * blocks * 144 + 4 * nl + 31) / 32), d_out = d.col(3 * nl);
  hip_ok(ops_of(H2_BN254)->msm_small(d_pts.data(), d_sc.data(), ms.data(), (uint32_t)nl, work, d_out, d.s), "msm_small");
  std::vector<uint64_t> jac(12 * nl);
  hip_ok(hipMemcpyAsync(jac.data(), d_out, 96 * nl, hipMemcpyDeviceToHost, d.s), "hipMemcpyAsync(D2H)");
  d.sync();
  d.release(work);
  d.release(d_out);
  for (const void* p : d_pts) d.release(const_cast<void*>(p));
  for (const void* p : d_sc) d.release(const_cast<void*>(p));
  for (size_t q = 0; q < nl; q++) {
    const uint64_t* J = jac.data() + 12 * q;
    const Fq X = Fq::from_mont_limbs(J), Y = Fq::from_mont_limbs(J + 4), Z = Fq::from_mont_limbs(J + 8);
    if (Z.is_zero()) continue;
    const Fq zi = Z.inv(), zi2 = zi.sqr();
    G1& g = out[live[q]];
    g.x = X * zi2;
    g.y = Y * zi2 * zi;
    g.inf = false;
  }
  return out;
}

}  // namespace product
}  // namespace h2
