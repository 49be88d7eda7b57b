// h2_prover.hip -- the reference crate's product surface behind the C ABI (include/h2hip.h, "product surface"):
//   h2_setup / h2_generate_proof[s] / h2_verify_proof[s] / h2_simulate / h2_circuit_count
// = setup / wasm_generate_proof / wasm_verify_proof / wasm_simulate_circuit / get_circuit_count of
// /root/reference/circuits/src/wasm.rs:49,68,77,125,182, which call utils.rs:59-158 (generate_params, generate_keys,
// generate_proof[_with_instance], verify[_with_instance]) over halo2_proofs @6b43b6b's keygen_vk / keygen_pk /
// create_proof / verify_proof with KZG over BN254, GWC or SHPLONK openings and a Blake2b transcript (SURVEY.md
// App. A.4-A.8).  halo2_prover_amd/prover.py + verifier.py are the readable Python statement of the same thing and
// produce identical bytes; this file is the one a Rust or JS host links against.
//
// Orchestration is host C++; every column stays in HBM.  Per proof: 6 MSM phases (keygen's fixed + sigma columns,
// advice, permutation products, random polynomial, quotient pieces, opening witnesses) through msm_device_run, the
// Lagrange -> coefficient -> extended-coset transforms through ntt_enqueue, and between them ONE launch each for the
// permutation ratio, the whole quotient numerator (expr_kernel), all evaluations at x, each opening combination
// (h2_prover_kernels.hpp).  The host hashes the transcript, synthesises the (sparse) witness and draws the blinding
// scalars from the caller's RNG in the reference's order, so that under the same RNG stream the proof bytes are the
// reference's.
#include "h2_prove.hpp"
#include "h2_verify.hpp"

using namespace h2;
using namespace h2::plonk;
using namespace h2::product;

namespace {

// prove side: circuit with witness, public inputs as the reference passes them (wasm.rs:84-117)
Job job_for_proof(const Json& js, int idx) {
  Job j = make_circuit(idx);
  if (j.index == 0) {
    static_cast<CollatzCircuit&>(*j.circuit).set_sequence(js.array("x"));
  } else if (j.index == 1) {
    auto& c = static_cast<ArithmeticCircuit&>(*j.circuit);
    c.x = Fr::from_u64(js.u64("x"));
    c.y = Fr::from_u64(js.u64("y"));
    c.constant = Fr::from_u64(js.u64("constant"));
    c.has_witness = true;
    j.public_input = {Fr::from_u64(js.u64("constant")), Fr::from_u64(js.u64("z"))};     // wasm.rs:93-94
  } else {
    auto& c = static_cast<PoseidonCircuit&>(*j.circuit);
    const auto& x = js.array("x");
    if (x.size() != 2) fail(H2_EPROOF, "poseidon: x must hold two values");
    c.message[0] = Fr::from_u64(x[0]);
    c.message[1] = Fr::from_u64(x[1]);
    c.has_witness = true;
    auto it = js.scalars.find("output");
    if (it == js.scalars.end()) fail(H2_EPROOF, "poseidon: missing output");
    j.public_input = {Fr::from_hex(it->second.c_str())};                                   // wasm.rs:116 hex_to_fr(output)
  }
  return j;
}
// verify side: the empty circuit, public inputs recomputed (wasm.rs:128-168).  hash = false leaves the Poseidon circuit's
// public input, the hash of the message, to the caller (h2_verify_proofs computes a batch's hashes together)
Job job_for_verify(const Json& js, int idx, bool hash = true) {
  Job j = make_circuit(idx);
  if (j.index == 1) {
    j.public_input = {Fr::from_u64(js.u64("constant")), Fr::from_u64(js.u64("z"))};
  } else if (j.index == 2) {
    auto& c = static_cast<PoseidonCircuit&>(*j.circuit);
    const auto& x = js.array("x");
    if (x.size() != 2) fail(H2_EPROOF, "poseidon: x must hold two values");
    c.message[0] = Fr::from_u64(x[0]);
    c.message[1] = Fr::from_u64(x[1]);
    if (hash) j.public_input = {c.output()};
  }
  return j;
}

// Batches of at least this many Poseidon items get their public inputs from ONE h2_poseidon_hash_device launch and one
// read-back instead of `count` host permutations (DESIGN.md section 7.14 has the measurement behind the number)
constexpr size_t POSEIDON_VERIFY_MIN = 64;
size_t g_poseidon_verify_min = POSEIDON_VERIFY_MIN;

// the public inputs of Poseidon jobs whose messages are set: Poseidon(message) over bn256::Fr with (8, 60), the same value
// c.output() computes
void poseidon_public_inputs(DevCtx* ctx, std::vector<Job>& jobs) {
  if (jobs.size() < g_poseidon_verify_min) {
    for (Job& j : jobs) j.public_input = {static_cast<PoseidonCircuit&>(*j.circuit).output()};
    return;
  }
  Dev d(ctx);
  std::vector<Fr> msgs;
  msgs.reserve(2 * jobs.size());
  for (Job& j : jobs) {
    const auto& c = static_cast<PoseidonCircuit&>(*j.circuit);
    msgs.push_back(c.message[0]);
    msgs.push_back(c.message[1]);
  }
  Col d_msgs = d.upload_frs(msgs);
  Col d_out = d.col(jobs.size());
  if (int rc = h2_poseidon_hash_device(H2_BN254, 8, 60, d_msgs, 2, 2, jobs.size(), d_out, d.s); rc != H2_OK)
    fail(rc, "poseidon public inputs: " + g_h2.last_error);
  const std::vector<Fr> out = d.download_frs(d_out, jobs.size());
  for (size_t i = 0; i < jobs.size(); i++) jobs[i].public_input = {out[i]};
}

template <class F>
int guarded(F&& body) {
  std::lock_guard<std::recursive_mutex> lk(g_h2_mu);
  try {
    return body();
  } catch (const Fail& f) {
    g_h2.last_error = f.what;
    return f.status;
  } catch (const std::exception& e) {
    g_h2.last_error = e.what();
    return H2_EPROOF;
  }
}

// 64 canonical little-endian bytes x || y -> the point; all zero = the identity
G1 g1_from_canonical(const uint8_t* p) {
  G1 g;
  Fq::from_le_bytes_canonical(p, &g.x);
  Fq::from_le_bytes_canonical(p + 32, &g.y);
  g.inf = g.x.is_zero() && g.y.is_zero();
  return g;
}

int emit(const std::vector<uint8_t>& data, uint8_t* out, size_t cap, size_t* out_len) {
  if (out_len) *out_len = data.size();
  if (!out || cap < data.size()) return H2_EINVAL;      // *out_len says how much is needed
  memcpy(out, data.data(), data.size());
  return H2_OK;
}

// what = 10 / 11 of h2_selftest_host: the host instantiations of pasta_decompress and base_sqrt over the base field FB of `ops`
template <class FB>
static int sqrt_selftest(const CurveOps* ops, int what, const uint8_t* in, size_t n, std::vector<uint8_t>& r) {
  for (size_t i = 0; i < n; i++) {
    uint8_t b[65];
    if (what == 10) {
      if (!ops->selftest_pasta_decompress) return H2_EINVAL;
      uint64_t aff[8];
      const int st = ops->selftest_pasta_decompress(in + 32 * i, aff);
      HF<FB>::from_mont_limbs(aff).to_le_bytes(b);
      HF<FB>::from_mont_limbs(aff + 4).to_le_bytes(b + 32);
      b[64] = (uint8_t)st;
      r.insert(r.end(), b, b + 65);
    } else {
      // a canonical element goes in as its Montgomery limbs; anything else as the bytes it is, for the routine to refuse
      uint64_t a[4], root[4];
      HF<FB> e;
      if (HF<FB>::from_le_bytes_canonical(in + 32 * i, &e)) memcpy(a, e.v.v, 32);
      else memcpy(a, in + 32 * i, 32);
      const int st = ops->selftest_base_sqrt(a, root);
      HF<FB>::from_mont_limbs(root).to_le_bytes(b);
      b[32] = (uint8_t)st;
      r.insert(r.end(), b, b + 33);
    }
  }
  return H2_OK;
}

}  // namespace

extern "C" {

int h2_circuit_count(void) { return 3; }      // wasm.rs:182

int h2_simulate(const char* json, int circuit, char* out, size_t cap, size_t* out_len) {
  return guarded([&]() -> int {
    std::string r;
    if (circuit == 0) {
      r = "N/A";                                                    // collatz.rs:248-250
    } else {
      const Json js(json);
      if (circuit == 1) {
        // (x * x) * (y * y) + constant in u64 arithmetic (arithmetic_circuit.rs:298-301; the reference panics on overflow)
        const unsigned __int128 x = js.u64("x"), y = js.u64("y"), c = js.u64("constant");
        const unsigned __int128 xx = x * x, yy = y * y;
        if (xx >> 64 || yy >> 64) fail(H2_EPROOF, "u64 overflow");
        const unsigned __int128 p = xx * yy;
        if (p >> 64 || (p + c) >> 64) fail(H2_EPROOF, "u64 overflow");
        r = std::to_string((uint64_t)(p + c));
      } else {
        PoseidonCircuit c;
        const auto& x = js.array("x");
        if (x.size() != 2) fail(H2_EPROOF, "poseidon: x must hold two values");
        c.message[0] = Fr::from_u64(x[0]);
        c.message[1] = Fr::from_u64(x[1]);
        r = "0x" + c.output().hex64();                               // format!("{:?}", Fr)
      }
    }
    if (out_len) *out_len = r.size();
    if (!out || cap < r.size() + 1) return H2_EINVAL;
    memcpy(out, r.c_str(), r.size() + 1);
    return H2_OK;
  });
}

int h2_setup(uint32_t k, h2_rng_fill_t rng_fn, void* rng_ctx, uint8_t* out, size_t cap, size_t* out_len) {
  return guarded([&]() -> int {
    if (k < 1 || k > 24) return H2_EINVAL;
    const size_t n = (size_t)1 << k, total = 4 + 128 * n + 256;
    if (out_len) *out_len = total;
    if (!out || cap < total) return H2_EINVAL;
    DevCtx* ctx = the_ctx();
    Dev d(ctx);
    Rng rng{rng_fn, rng_ctx};
    const Fr s = rng.fr_random();
    // g[i] = [s^i] G
    Col g = d.col(2 * n), gl = d.col(2 * n);
    uint64_t sl[4];
    Dev::limbs(s, sl);
    hip_ok(d.ops->srs_powers(g, sl, (uint32_t)n, d.s), "srs_powers");
    // g_lagrange[i] = [L_i(s)] G with L_i(s) = w^i (s^n - 1) / (n (s - w^i))
    Domain D(3, k);
    const Fr sn = s.pow_u64(n);
    Col lag = d.col(n);
    if (sn == Fr::one()) {             // s on the domain (never in practice): L_i(s) is an indicator
      std::vector<SparseCol> ind(1);
      Fr w = Fr::one();
      for (uint32_t i = 0; i < n; i++) {
        if (w == s) ind[0][i] = Fr::one();
        w *= D.omega;
      }
      d.fill_sparse(lag, n, ind);
    } else {
      // ws = w^i ; den = s - w^i ; lag = ws / den * (s^n - 1) / n
      Col ws = d.col(n), den = d.col(n);
      std::vector<SparseCol> c1(1);
      c1[0][0] = Fr::one();
      d.fill_sparse(ws, n, c1);
      d.ntt(ws, 1, D.omega, k);                                     // ones
      d.copy(den, ws, n * 32);
      uint64_t w[4];
      Dev::limbs(D.omega, w);
      hip_ok(d.ops->poly_powers(ws, n, 1, w, d.s), "poly_powers");
      d.lincomb(den, (uint32_t)n, {{den, s}, {ws, -Fr::one()}});
      hip_ok(d.ops->poly_inverse(den, n, d.s), "poly_inverse");
      hip_ok(d.ops->poly_pointwise(den, ws, n, 2, d.s), "poly_pointwise");
      d.lincomb(lag, (uint32_t)n, {{den, (sn - Fr::one()) * D.n_inv}});
    }
    hip_ok(d.ops->fixed_base_mul(gl, lag, (uint32_t)n, d.s), "fixed_base_mul");
    memcpy(out, &k, 4);
    hip_ok(hipMemcpyAsync(out + 4, g, 64 * n, hipMemcpyDeviceToHost, d.s), "D2H");
    hip_ok(hipMemcpyAsync(out + 4 + 64 * n, gl, 64 * n, hipMemcpyDeviceToHost, d.s), "D2H");
    // g2 and [s] g2
    bn::G2 g2;
    g2.x = {Fq::from_hex("0x1800deef121f1e76426a00665e5c4479674322d4f75edadd46debd5cd992f6ed"),
            Fq::from_hex("0x198e9393920d483a7260bfb731fb5d25f1aa493335a9e71297e485b7aef312c2")};
    g2.y = {Fq::from_hex("0x12c85ea5db8c6deb4aab71808dcb408fe3d1e7690c43d37b4ce6cc0166fa7daa"),
            Fq::from_hex("0x090689d0585ff075ec9e99ad690c3395bc4b313370b38ef355acdadcd122975b")};
    g2.inf = false;
    const bn::G2 s_g2 = g2_mul(s, g2);
    uint8_t* t = out + 4 + 128 * n;
    const Fq* parts[8] = {&g2.x.a, &g2.x.b, &g2.y.a, &g2.y.b, &s_g2.x.a, &s_g2.x.b, &s_g2.y.a, &s_g2.y.b};
    for (int i = 0; i < 8; i++) memcpy(t + 32 * i, parts[i]->v.v, 32);
    d.sync();
    return H2_OK;
  });
}

// Params::downsize(k): g truncated, g_lagrange recomputed from it (h2_g_to_lagrange_device), the G2 tail copied
int h2_params_downsize(const uint8_t* params, size_t params_len, uint32_t k, uint8_t* out, size_t cap, size_t* out_len) {
  return guarded([&]() -> int {
    DevCtx* ctx = the_ctx();
    if (!params || params_len < 4) fail(H2_EPROOF, "params: truncated");
    uint32_t k0;
    memcpy(&k0, params, 4);
    if (k0 > 28) fail(H2_EPROOF, "params: k out of range");
    const size_t n0 = (size_t)1 << k0;
    if (params_len != 4 + 128 * n0 + 256) fail(H2_EPROOF, "params: wrong length for k");
    if (k < 1 || k > k0 || k > 26) return H2_EINVAL;
    const size_t n = (size_t)1 << k, total = 4 + 128 * n + 256;
    if (out_len) *out_len = total;
    if (!out || cap < total) return H2_EINVAL;
    Dev d(ctx);
    const Domain D(2, k);
    uint64_t w[4], c[4];
    Dev::limbs(D.omega_inv, w);
    Dev::limbs(D.n_inv, c);
    Col g = d.col(2 * n);
    hip_ok(hipMemcpyAsync(g, params + 4, 64 * n, hipMemcpyHostToDevice, d.s), "H2D");
    st_ok(h2_g_to_lagrange_device(H2_BN254, g, k, w, c, g, d.s), "h2_g_to_lagrange_device");
    hip_ok(hipMemcpyAsync(out + 4 + 64 * n, g, 64 * n, hipMemcpyDeviceToHost, d.s), "D2H");
    memcpy(out, &k, 4);
    memmove(out + 4, params + 4, 64 * n);
    memcpy(out + 4 + 128 * n, params + 4 + 128 * n0, 256);
    d.sync();
    return H2_OK;
  });
}

int h2_generate_proof(const uint8_t* params, size_t params_len, const char* json, int circuit, h2_rng_fill_t rng_fn,
                      void* rng_ctx, uint8_t* out, size_t cap, size_t* out_len) {
  return guarded([&]() -> int {
    Trace trace("generate_proof");
    DevCtx* ctx = the_ctx();
    const Params& P = params_get(params, params_len);
    trace.mark("params");
    const Json js(json);
    Job job = job_for_proof(js, circuit);
    trace.mark("job");
    // the key comes from the EMPTY circuit (wasm.rs:86,95,114 rebuild it on every call; here it is kept, see
    // h2_key_cache), the witness from the JSON
    std::unique_ptr<ProvingKey> owner;
    ProvingKey& K = key_for(P, job.index, ctx, owner);
    trace.mark("key");
    // a batch of one: the witness is synthesised and checked before a random byte is drawn or anything is enqueued
    std::vector<Witness> items;
    items.push_back({&job.public_input, synthesize_checked(*job.circuit, job.public_input, K.dom->n, K.bf), Rng{rng_fn, rng_ctx}});
    const std::vector<std::vector<uint8_t>> proofs = create_proofs(K, items, trace);
    trace.mark("create_proof");
    return emit(proofs[0], out, cap, out_len);
  });
}

int h2_generate_proofs(const uint8_t* params, size_t params_len, size_t count, const char* const* jsons, int circuit,
                       h2_rng_fill_t rng_fn, void* const* rng_ctxs, uint8_t* out, size_t cap, size_t* proof_lens,
                       size_t* out_len) {
  return guarded([&]() -> int {
    Trace trace("generate_proofs");
    DevCtx* ctx = the_ctx();
    if (count && (!jsons || !out_len || !proof_lens)) return H2_EINVAL;
    if (count == 0) {
      if (out_len) *out_len = 0;
      return H2_OK;
    }
    const Params& P = params_get(params, params_len);
    // every JSON parsed and every witness synthesised before anything is enqueued: a bad item ends the call here
    std::vector<Job> jobs;
    for (size_t i = 0; i < count; i++) jobs.push_back(job_for_proof(Json(jsons[i]), circuit));
    std::unique_ptr<ProvingKey> owner;
    ProvingKey& K = key_for(P, jobs[0].index, ctx, owner);
    std::vector<Witness> items;
    for (size_t i = 0; i < count; i++)
      items.push_back({&jobs[i].public_input, synthesize_checked(*jobs[i].circuit, jobs[i].public_input, K.dom->n, K.bf),
                       Rng{rng_fn, rng_ctxs ? rng_ctxs[i] : nullptr}});
    trace.mark("params, jobs, key, witnesses");
    // every proof of a circuit has the plan's length: the room is checked before a random byte is drawn
    const size_t each = 32 * ((size_t)K.plan.leading + K.plan.evals.size() + K.plan.opening_points);
    *out_len = each * count;
    if (!out || cap < each * count) return H2_EINVAL;
    const std::vector<std::vector<uint8_t>> proofs = create_proofs(K, items, trace);
    trace.mark("create_proofs");
    size_t total = 0;
    for (auto& pr : proofs) total += pr.size();
    if (total != each * count) fail(H2_EDEVICE, "a proof's length is not its plan's");
    uint8_t* at = out;
    for (size_t i = 0; i < count; i++) {
      proof_lens[i] = proofs[i].size();
      memcpy(at, proofs[i].data(), proofs[i].size());
      at += proofs[i].size();
    }
    return H2_OK;
  });
}

int h2_verify_proof(const uint8_t* params, size_t params_len, const uint8_t* proof, size_t proof_len, const char* json,
                    int circuit, int* ok) {
  if (ok) *ok = 0;
  return guarded([&]() -> int {
    if (!ok || (!proof && proof_len)) return H2_EINVAL;
    DevCtx* ctx = the_ctx();
    const Params& P = params_get(params, params_len);
    const Json js(json);
    Job job = job_for_verify(js, circuit);
    std::unique_ptr<ProvingKey> owner;
    ProvingKey& K = key_for(P, job.index, ctx, owner);
    *ok = verify_proof(K, proof, proof_len, job.public_input) ? 1 : 0;
    return H2_OK;
  });
}

int h2_verify_proofs(const uint8_t* params, size_t params_len, size_t count, const uint8_t* const* proofs,
                     const size_t* proof_lens, const char* const* jsons, int circuit, h2_rng_fill_t rng_fn, void* rng_ctx,
                     int* ok, int* all_ok) {
  if (all_ok) *all_ok = 0;
  if (ok)
    for (size_t i = 0; i < count; i++) ok[i] = 0;
  return guarded([&]() -> int {
    if (count && (!ok || !proofs || !proof_lens || !jsons)) return H2_EINVAL;
    for (size_t i = 0; i < count; i++)
      if (!proofs[i] && proof_lens[i]) return H2_EINVAL;
    Trace trace("verify_proofs");
    DevCtx* ctx = the_ctx();
    if (count == 0) {
      if (all_ok) *all_ok = 1;
      return H2_OK;
    }
    const Params& P = params_get(params, params_len);
    std::vector<Job> jobs;
    for (size_t i = 0; i < count; i++) jobs.push_back(job_for_verify(Json(jsons[i]), circuit, false));
    trace.mark("params, jobs");
    if (jobs[0].index == 2) poseidon_public_inputs(ctx, jobs);
    trace.mark("poseidon hashes");
    std::unique_ptr<ProvingKey> owner;
    ProvingKey& K = key_for(P, jobs[0].index, ctx, owner);
    trace.mark("key");
    if (bn::g2_on_curve(P.g2) && bn::g2_on_curve(P.s_g2)) {        // otherwise no proof verifies under these params
      Rng rng{rng_fn, rng_ctx};
      for (size_t g0 = 0; g0 < count; g0 += VERIFY_GROUP) {
        const size_t cnt = std::min(VERIFY_GROUP, count - g0);
        verify_group(K, cnt, proofs + g0, proof_lens + g0, jobs.data() + g0, rng, ok + g0, trace);
      }
    }
    int all = 1;
    for (size_t i = 0; i < count; i++) all &= ok[i];
    if (all_ok) *all_ok = all;
    return H2_OK;
  });
}

uint64_t h2_selftest_pairing_checks(void) {
  std::lock_guard<std::recursive_mutex> lk(g_h2_mu);
  return g_pairing_checks;
}

// forget the resident SRS tables (the next call with any params blob parses and registers it again)
int h2_params_cache_clear(void) {
  return guarded([&]() -> int {
    g_keys.clear();                                   // keys point into the params list
    for (auto& p : g_params) {
      (void)h2_bases_release(p.h_g);
      (void)h2_bases_release(p.h_gl);
    }
    g_params.clear();
    return H2_OK;
  });
}

// called by h2_shutdown: drop keys, params and the cached device blocks
void h2_prover_shutdown(void) {
  g_keys.clear();
  g_kits.clear();
  for (auto& p : g_params) {
    (void)h2_bases_release(p.h_g);
    (void)h2_bases_release(p.h_gl);
  }
  g_params.clear();
  for (auto& kv : Dev::cache()) {
    DeviceGuard dg(kv.first.first);
    (void)hipFree(kv.second);
  }
  Dev::cache().clear();
}

// commit phases that were spread over more than one context since the library was loaded (tests)
uint64_t h2_selftest_sharded_commits(void) {
  std::lock_guard<std::recursive_mutex> lk(g_h2_mu);
  return g_sharded_commits;
}

// commit_begin calls since the library was loaded: a lockstep batch makes as many as one proof, N calls N times as many
uint64_t h2_selftest_commit_launches(void) {
  std::lock_guard<std::recursive_mutex> lk(g_h2_mu);
  return g_commit_launches;
}

// test hook: proofs per lockstep group of h2_generate_proofs (0 restores the default)
int h2_selftest_set_prove_group(size_t proofs) {
  std::lock_guard<std::recursive_mutex> lk(g_h2_mu);
  g_prove_group = proofs ? proofs : PROVE_GROUP;
  return H2_OK;
}

// test hook: Poseidon items from which h2_verify_proofs hashes on the device (0 restores the default)
int h2_selftest_set_poseidon_verify_min(size_t count) {
  std::lock_guard<std::recursive_mutex> lk(g_h2_mu);
  g_poseidon_verify_min = count ? count : POSEIDON_VERIFY_MIN;
  return H2_OK;
}

// test hook: rows per context from which a commit phase is spread over the contexts (0 restores the default)
int h2_selftest_set_shard_min_rows(size_t rows) {
  std::lock_guard<std::recursive_mutex> lk(g_h2_mu);
  g_shard_min_rows = rows ? rows : 1024;
  return H2_OK;
}

// keep proving keys between calls (default) or rebuild them on every call as the reference does; returns the old setting
int h2_key_cache(int enable) {
  std::lock_guard<std::recursive_mutex> lk(g_h2_mu);
  const int old = g_key_cache ? 1 : 0;
  g_key_cache = enable != 0;
  if (!g_key_cache) g_keys.clear();
  return old;
}

// host-side pieces exposed for the CPU tests (no GPU needed): the vk digest of a circuit for given commitments, the
// Poseidon constants, Blake2b, the pairing
int h2_selftest_host(int what, const uint8_t* in, size_t in_len, uint8_t* out, size_t cap, size_t* out_len) {
  return guarded([&]() -> int {
    std::vector<uint8_t> r;
    if (what == 0) {                       // Blake2b-512 with the transcript personalisation
      Blake2b h("Halo2-Transcript");
      h.update(in, in_len);
      r.resize(64);
      h.digest(r.data());
    } else if (what == 1) {                // Poseidon constants: 68 x 3 round constants, mds, minv (canonical LE)
      const PoseidonConstants& pc = poseidon_constants();
      auto put = [&](const Fr& f) {
        uint8_t b[32];
        f.to_le_bytes(b);
        r.insert(r.end(), b, b + 32);
      };
      for (auto& row : pc.rcs)
        for (auto& v : row) put(v);
      for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) put(pc.mds[i][j]);
      for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) put(pc.minv[i][j]);
    } else if (what == 2 || what == 3 || what == 4) {   // vk Debug string of circuit (what - 2) for k = in[0] and the given
      const int idx = what - 2;                         // commitments (64-byte canonical x || y each, zero = identity)
      const std::unique_ptr<Circuit> c = make_circuit(idx).circuit;
      if (in_len < 1) return H2_EINVAL;
      const uint32_t k = in[0];
      Domain D((uint32_t)c->degree, k);
      const size_t nfx = (size_t)c->num_fixed, nsg = c->permutation_columns.size();
      if (in_len != 1 + 64 * (nfx + nsg)) return H2_EINVAL;
      auto pt = [&](size_t i) { return g1_from_canonical(in + 1 + 64 * i); };
      std::vector<G1> fc, sc;
      for (size_t i = 0; i < nfx; i++) fc.push_back(pt(i));
      for (size_t i = 0; i < nsg; i++) sc.push_back(pt(nfx + i));
      const std::string s = vk_debug_string(*c, k, D.ext_k, D.omega, fc, sc);
      const Fr repr = vk_transcript_repr(s);
      r.resize(32);
      repr.to_le_bytes(r.data());
      r.insert(r.end(), s.begin(), s.end());
    } else if (what == 6) {                // quotient program of circuit in[0]: u32 x 6 = instructions, products, column
      if (in_len != 1) return H2_EINVAL;   // reads, LDS slots, constants, inserted reductions; then the code (12 bytes each)
      ProvingKey K;
      K.circuit = make_circuit(in[0]).circuit;
      key_shape(K);
      build_quotient_program(K);
      r = K.prog.report();
    } else if (what == 7) {                // a caller's DAG (program_from_dag) compiled: what 6 reports, then the
      ExprProgram X;                       // constant table (32 canonical LE bytes each; the one compile adds included)
      program_from_dag(in, in_len, X);
      r = X.report_with_table();
    } else if (what == 8) {                // the decompression routine's host instantiation: n x 32 bytes -> n x (64 canonical
      if (in_len % 32) return H2_EINVAL;   // LE bytes x || y, one status byte)
      const CurveOps* ops = ops_of(H2_BN254);
      for (size_t i = 0; i < in_len / 32; i++) {
        uint64_t aff[8];
        const int st = ops->selftest_decompress(in + 32 * i, aff);
        uint8_t b[65];
        Fq::from_mont_limbs(aff).to_le_bytes(b);
        Fq::from_mont_limbs(aff + 4).to_le_bytes(b + 32);
        b[64] = (uint8_t)st;
        r.insert(r.end(), b, b + 65);
      }
    } else if (what == 10 || what == 11) { // pasta_decompress / base_sqrt on the host: one curve byte, then n x 32 bytes ->
      if (in_len < 1 || (in_len - 1) % 32 || !curve_ok(in[0])) return H2_EINVAL;   // n x (64 + 1) / n x (32 + 1) bytes
      const CurveOps* ops = ops_of(in[0]);
      const size_t n = (in_len - 1) / 32;
      const int rc = in[0] == H2_BN254    ? sqrt_selftest<BN254_CURVE::Base>(ops, what, in + 1, n, r)
                     : in[0] == H2_PALLAS ? sqrt_selftest<PALLAS_CURVE::Base>(ops, what, in + 1, n, r)
                                          : sqrt_selftest<VESTA_CURVE::Base>(ops, what, in + 1, n, r);
      if (rc != H2_OK) return rc;
    } else if (what == 5) {                // pairing check on two (G1, G2) pairs: 2 x (64 + 128) canonical bytes -> 1 byte
      if (in_len != 2 * 192) return H2_EINVAL;
      std::vector<std::pair<G1, bn::G2>> pairs;
      for (int i = 0; i < 2; i++) {
        const uint8_t* p = in + 192 * i;
        const G1 g = g1_from_canonical(p);
        bn::G2 q;
        Fq::from_le_bytes_canonical(p + 64, &q.x.a);
        Fq::from_le_bytes_canonical(p + 96, &q.x.b);
        Fq::from_le_bytes_canonical(p + 128, &q.y.a);
        Fq::from_le_bytes_canonical(p + 160, &q.y.b);
        q.inf = q.x.is_zero() && q.y.is_zero();
        if (!bn::g2_on_curve(q)) return H2_EPROOF;
        pairs.push_back({g, q});
      }
      r.push_back(bn::pairing_check(pairs) ? 1 : 0);
    } else if (what == 9) {                // the opening plan of circuit in[0] at k = in[1] (OpeningPlan::dump), built as
      if (in_len != 2 || in[1] > 28) return H2_EINVAL;    // keygen builds it: host only
      ProvingKey K;
      Job made = make_circuit(in[0]);
      K.circuit = std::move(made.circuit);
      key_shape(K);
      r = opening_plan(*K.circuit, K.sets, K.bf, in[1], made.shplonk).dump();
    } else {
      return H2_EINVAL;
    }
    return emit(r, out, cap, out_len);
  });
}

// a caller's DAG (program_from_dag) run by expr_kernel over en = 2^log_en rows, launched as create_proof launches it
int h2_selftest_expr_run(const uint8_t* dag, size_t dag_len, const uint64_t* cols, const uint32_t* log_len, uint32_t ncols,
                         uint32_t log_en, uint32_t step, uint64_t* out, uint32_t stats[6]) {
  return guarded([&]() -> int {
    if (!cols || !log_len || !out || !stats || ncols == 0 || ncols > (1u << 16) || log_en > 22) return H2_EINVAL;
    ExprProgram X;
    program_from_dag(dag, dag_len, X);
    (void)expr_lds_bytes(X);                 // over the LDS limit: refused before a device is even looked at
    for (auto& nd : X.nodes)
      if (nd.op == 1 && (uint32_t)nd.col >= ncols) fail(H2_EINVAL, "dag: no such column");
    size_t total = 0;
    for (uint32_t c = 0; c < ncols; c++) {
      if (log_len[c] > 24) return H2_EINVAL;
      total += (size_t)1 << log_len[c];
    }
    if (total > ((size_t)1 << 24)) return H2_EINVAL;
    // the kernel takes every column element as canonical (x 2^256 mod p below p): anything else is refused here
    uint64_t p[4];
    for (int w = 0; w < 4; w++) p[w] = (uint64_t)BN254_FR::P(2 * w) | ((uint64_t)BN254_FR::P(2 * w + 1) << 32);
    for (size_t e = 0; e < total; e++) {
      const uint64_t* v = cols + 4 * e;
      int w = 3;
      while (w > 0 && v[w] == p[w]) w--;
      if (v[w] >= p[w]) return H2_EINVAL;
    }
    const uint32_t en = 1u << log_en;
    const std::vector<uint8_t> rep = X.report();
    memcpy(stats, rep.data(), 24);
    Dev d(the_ctx());
    const pk::XInstr* d_code = (const pk::XInstr*)d.upload(X.code.data(), X.code.size() * sizeof(pk::XInstr));
    const U128* d_cols = (const U128*)d.upload(cols, total * 32);
    std::vector<const U128*> ptrs(ncols);
    std::vector<uint32_t> masks(ncols);
    size_t off = 0;
    for (uint32_t c = 0; c < ncols; c++) {
      ptrs[c] = d_cols + 2 * off;
      masks[c] = (1u << log_len[c]) - 1;
      off += (size_t)1 << log_len[c];
    }
    Col d_out = d.col(en);
    expr_launch(d, X, d_code, ptrs, masks, X.consts, X.consts.size(), d_out, step, en, 1);
    hip_ok(hipMemcpyAsync(out, d_out, (size_t)en * 32, hipMemcpyDeviceToHost, d.s), "hipMemcpyAsync(D2H)");
    d.sync();
    return H2_OK;
  });
}

}  // extern "C"
