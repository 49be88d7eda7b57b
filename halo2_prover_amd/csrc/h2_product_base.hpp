// h2_product_base.hpp -- what every part of the product surface (h2_prover.hip) starts from: the error that carries a
// status code to the C ABI, phase timings, the caller's RNG, the JSON inputs.
#pragma once
#include <sys/random.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "h2_host.hpp"
#include "h2_internal.hpp"

namespace h2 {
namespace product {

struct Fail {
  int status;
  std::string what;
};
[[noreturn]] inline void fail(int status, const std::string& what) { throw Fail{status, what}; }
inline void hip_ok(hipError_t e, const char* where) {
  if (e != hipSuccess) fail(H2_EDEVICE, std::string(where) + ": " + hipGetErrorString(e));
}
inline void st_ok(int rc, const char* where) {
  if (rc != H2_OK) fail(rc, where);
}

// one kernel launch on `stream` (no dynamic LDS) and its launch status
template <class K, class... A>
void launch(const char* name, K kernel, dim3 grid, dim3 block, hipStream_t stream, A... args) {
  hipLaunchKernelGGL(kernel, grid, block, 0, stream, args...);
  hip_ok(hipGetLastError(), name);
}

// phase timings on stderr when H2_TRACE is set (wall clock, the stream is NOT synchronised for the marks)
struct Trace {
  bool on;
  std::chrono::steady_clock::time_point t0, last;
  const char* what;
  explicit Trace(const char* w) : on(getenv("H2_TRACE") != nullptr), what(w) { t0 = last = std::chrono::steady_clock::now(); }
  void mark(const char* phase) {
    if (!on) return;
    const auto now = std::chrono::steady_clock::now();
    fprintf(stderr, "[h2 %s] %-28s %8.3f ms (+%.3f)\n", what, phase, std::chrono::duration<double, std::milli>(now - t0).count(),
            std::chrono::duration<double, std::milli>(now - last).count());
    last = now;
  }
};

// ---- the caller's RNG, consumed call by call exactly as the reference's RngCore is -------------------------------
struct Rng {
  h2_rng_fill_t fn;
  void* ctx;
  void fill(uint8_t* out, size_t n) {
    if (fn) {
      fn(ctx, out, n);
      return;
    }
    size_t got = 0;
    while (got < n) {
      const ssize_t r = getrandom(out + got, n - got, 0);
      if (r <= 0) fail(H2_EDEVICE, "getrandom failed");
      got += (size_t)r;
    }
  }
  // Fr::random(rng): eight next_u64 calls, the 512-bit integer reduced mod r (halo2curves' from_bytes_wide)
  Fr fr_random() {
    uint8_t b[64];
    for (int i = 0; i < 8; i++) fill(b + 8 * i, 8);
    return Fr::from_le_bytes_wide(b);
  }
};

// ---- the three JSON inputs (arithmetic_circuit.rs:39-45, collatz.rs:20-23, poseidon_circuit.rs:37-41) --------------
struct Json {
  std::map<std::string, std::string> scalars;              // "x": 6   or  "output": "0x.."
  std::map<std::string, std::vector<uint64_t>> arrays;     // "x": [1, 2]
  static uint64_t to_u64(const std::string& s) {
    if (s.empty()) fail(H2_EPROOF, "json: empty number");
    uint64_t v = 0;
    for (char c : s) {
      if (c < '0' || c > '9') fail(H2_EPROOF, "json: not an unsigned integer");
      if (v > (~0ull - (uint64_t)(c - '0')) / 10) fail(H2_EPROOF, "json: integer exceeds u64");
      v = v * 10 + (uint64_t)(c - '0');
    }
    return v;
  }
  explicit Json(const char* s) {
    if (!s) fail(H2_EINVAL, "json: null");
    const char* p = s;
    auto ws = [&] { while (*p == ' ' || *p == '\n' || *p == '\t' || *p == '\r') p++; };
    auto token = [&] {   // a bare number or a quoted string
      ws();
      std::string t;
      if (*p == '"') {
        p++;
        while (*p && *p != '"') t += *p++;
        if (*p != '"') fail(H2_EPROOF, "json: unterminated string");
        p++;
      } else {
        while ((*p >= '0' && *p <= '9') || *p == '-' || *p == '.') t += *p++;
      }
      return t;
    };
    ws();
    if (*p != '{') fail(H2_EPROOF, "json: expected an object");
    p++;
    for (;;) {
      ws();
      if (*p == '}') break;
      if (*p != '"') fail(H2_EPROOF, "json: expected a key");
      const std::string key = token();
      ws();
      if (*p != ':') fail(H2_EPROOF, "json: expected ':'");
      p++;
      ws();
      if (*p == '[') {
        p++;
        std::vector<uint64_t> arr;
        for (;;) {
          ws();
          if (*p == ']') { p++; break; }
          arr.push_back(to_u64(token()));
          ws();
          if (*p == ',') p++;
        }
        arrays[key] = arr;
      } else if (strncmp(p, "null", 4) == 0) {
        p += 4;
      } else {
        scalars[key] = token();
      }
      ws();
      if (*p == ',') p++;
      else if (*p != '}') fail(H2_EPROOF, "json: expected ',' or '}'");
    }
  }
  uint64_t u64(const std::string& k) const {
    auto it = scalars.find(k);
    if (it == scalars.end()) fail(H2_EPROOF, "json: missing field " + k);
    return to_u64(it->second);
  }
  const std::vector<uint64_t>& array(const std::string& k) const {
    auto it = arrays.find(k);
    if (it == arrays.end()) fail(H2_EPROOF, "json: missing array " + k);
    return it->second;
  }
};

}  // namespace product
}  // namespace h2
