"""h2_generate_proofs against N one-witness calls of h2_generate_proof: arithmetic at k = 4, Poseidon at k = 6, 11 and 16, Collatz
(SHPLONK) at k = 10, N = 1 .. 32 proofs.  Writes profiles/prove_batch_times.json (or --out FILE) and prints the table of
DESIGN.md section 7.3.

One process, key cached.  Per (circuit, N): milliseconds for the loop of N one-witness calls (the same prover with a
batch of one: what a host that does not batch pays) and for one batch call, each the best of five with the spread
(max - min) of the five; the proofs of every timed call of either route are compared byte for byte -- proof i draws from
its own recorded stream in both -- and item 0 with the recorded proof's hash.  The streams reach the library through a Python callback,
which costs both routes the same per proof; the `os` columns repeat the timing with OS randomness (no callback, no
byte comparison), and one more batch call per row runs under H2_TRACE for its phase marks.

Exits non-zero when a comparison fails, when a batch of one is slower than the one-witness call by more than the loop's
spread, or when at N = 16 the batch is not below the loop by more than that spread.  No ratio is fixed in advance.
"""
import argparse
import ctypes
import hashlib
import json
import os
import re
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import halo2_prover_amd as h2  # noqa: E402
from halo2_prover_amd import lib as h2lib  # noqa: E402

SIZES = (1, 2, 4, 8, 16, 32)
BOUND_N = 16
# (circuit, index, k, SHA-256 of the proof recorded for the first input under the stream behind setup(k))
CONFIGS = (
    ("arithmetic", 1, 4, "31d427b9666777794f4a126fbde11584f28748005a32dcaf27e40974f3866f13"),
    ("poseidon", 2, 6, "6d235bf4637e1dce12559c44eaf77812bae2746d78331db3850e16b26234e63e"),
    ("collatz", 0, 10, "8709c25ae65667b14921a4df48907cccc0d7d024ae2f56b2e9e25b6b4d679352"),
    ("poseidon", 2, 11, "8d2d9052b47d9c9b45f3e3c268cec30797f74990cb47367bdfa7fbe77832129c"),
    ("poseidon", 2, 16, "4c4e7d9301b652969a92718b3183f0bda79be2aaab245b68033ca96bf27bdc3c"),
)
POSEIDON_0 = '{"x":[1,2],"output":"0x152e960b5c9c8a624b2cdf4855250e8a54ee074254281310dc4a9704f78c1917"}'
COLLATZ_0 = [9, 28, 14, 7, 22, 11, 34, 17, 52, 26, 13, 40, 20, 10, 5, 16, 8, 4, 2, 1]
DIGESTS = 2048           # calls one recorded stream can serve


class Streams:
    """the recorded RNG stream (call c fills its buffer from SHA256("seed0-" + str(c)), at most 32 bytes a call), one
    per proof: ctx = i + 1 draws from stream i.  The digests are made ahead so that a call is one memmove."""

    def __init__(self, starts):
        self.starts = list(starts)
        self.tables = [ctypes.create_string_buffer(b"".join(hashlib.sha256(b"seed0-%d" % (s + c)).digest() for c in range(DIGESTS)),
                                                   32 * DIGESTS) for s in self.starts]
        self.base = [ctypes.addressof(t) for t in self.tables]
        self.at = [0] * len(self.starts)

        def fill(ctx, out, n):
            i = ctx - 1
            assert n <= 32 and self.at[i] < DIGESTS
            ctypes.memmove(out, self.base[i] + 32 * self.at[i], n)
            self.at[i] += 1
        self.cb = h2lib.RNG_FILL(fill)
        self.ctxs = (ctypes.c_void_p * len(self.starts))(*range(1, len(self.starts) + 1))

    def rewind(self):
        self.at = [0] * len(self.starts)

    def used(self, i):
        return self.at[i]


def setup(L, k):
    """h2_setup under the recorded stream from its start -> (params, calls the setup consumed)"""
    s = Streams([0])
    cap = 4 + 128 * (1 << k) + 256
    buf = ctypes.create_string_buffer(cap)
    n = ctypes.c_size_t(0)
    h2lib.check(L.h2_setup(k, s.cb, 1, buf, cap, ctypes.byref(n)), "h2_setup")
    return buf.raw[:n.value], s.used(0)


def inputs(L, circuit, count):
    """`count` distinct JSON inputs, the recorded one first"""
    if circuit == "arithmetic":
        out = ['{"x":6,"y":9,"constant":7,"z":2923}']
        for i in range(1, count):
            x, y, c = 11 + i, 3 * i + 2, 1000 + i
            out.append('{"x":%d,"y":%d,"constant":%d,"z":%d}' % (x, y, c, x * x * y * y + c))
        return out
    if circuit == "poseidon":
        out = [POSEIDON_0]
        buf = ctypes.create_string_buffer(256)
        n = ctypes.c_size_t(0)
        for i in range(1, count):
            msg = (1000 + i, 7 * i + 3)
            h2lib.check(L.h2_simulate(('{"x":[%d,%d]}' % msg).encode(), 2, buf, 256, ctypes.byref(n)), "h2_simulate")
            out.append('{"x":[%d,%d],"output":"%s"}' % (msg[0], msg[1], buf.value.decode()))
        return out
    out, start = ['{"x":%s}' % str(COLLATZ_0).replace(" ", "")], 2
    while len(out) < count:
        start += 1
        seq = [start]
        while seq[-1] != 1:
            seq.append(seq[-1] // 2 if seq[-1] % 2 == 0 else 3 * seq[-1] + 1)
        if len(seq) <= 32 and seq != COLLATZ_0:
            out.append('{"x":%s}' % str(seq).replace(" ", ""))
    return out


class Row:
    def __init__(self, L, params, jsons, idx, first):
        n = len(jsons)
        self.L, self.params, self.idx, self.n = L, params, idx, n
        self.texts = [j.encode() for j in jsons]
        self.jsons = (ctypes.c_char_p * n)(*self.texts)
        self.streams = Streams([first] + [first + 1000 * i for i in range(1, n)])
        self.cap = n << 13
        self.out = ctypes.create_string_buffer(self.cap)
        self.lens = (ctypes.c_size_t * n)()
        self.total = ctypes.c_size_t(0)
        self.one = ctypes.create_string_buffer(1 << 13)

    def batch(self, recorded=True):
        s = self.streams
        s.rewind()
        h2lib.check(self.L.h2_generate_proofs(self.params, len(self.params), self.n, self.jsons, self.idx, s.cb if recorded else None,
                                              s.ctxs if recorded else None, self.out, self.cap, self.lens, ctypes.byref(self.total)),
                    "h2_generate_proofs")
        raw, proofs, at = self.out.raw, [], 0
        for ln in self.lens:
            proofs.append(raw[at:at + ln])
            at += ln
        return proofs

    def loop(self, recorded=True):
        s = self.streams
        s.rewind()
        proofs = []
        ln = ctypes.c_size_t(0)
        for i, js in enumerate(self.texts):
            h2lib.check(self.L.h2_generate_proof(self.params, len(self.params), js, self.idx, s.cb if recorded else None,
                                                 i + 1 if recorded else None, self.one, 1 << 13, ctypes.byref(ln)), "h2_generate_proof")
            proofs.append(self.one.raw[:ln.value])
        return proofs


def timed(fn, repeats=5):
    """-> (best ms, spread ms of the `repeats` runs, the results of every run)"""
    times, results = [], []
    for _ in range(repeats):
        t = time.perf_counter()
        res = fn()
        times.append((time.perf_counter() - t) * 1e3)
        results.append(res)
    return min(times), max(times) - min(times), results


def traced(fn):
    """fn() with H2_TRACE set and this process's stderr caught -> {phase: ms}"""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as tmp:
        os.dup2(tmp.fileno(), 2)
        os.environ["H2_TRACE"] = "1"
        try:
            fn()
        finally:
            del os.environ["H2_TRACE"]
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        text = tmp.read().decode(errors="replace")
    phases = {}
    for line in text.splitlines():
        m = re.match(r"\[h2 generate_proofs\] (.+?)\s+[0-9.]+ ms \(\+([0-9.]+)\)", line)
        if m:
            phases[m.group(1)] = round(phases.get(m.group(1), 0.0) + float(m.group(2)), 3)
    return phases


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prove_batch_times.json"))
    ap.add_argument("--sizes", default=",".join(str(s) for s in SIZES))
    ap.add_argument("--rows", default="", help="comma-separated k values to run (default: all)")
    args = ap.parse_args()
    sizes = [int(s) for s in args.sizes.split(",")]
    only = {int(s) for s in args.rows.split(",") if s}
    h2.init(0)
    L = h2.load()
    import torch
    result = {"device": torch.cuda.get_device_name(0), "h2_version": L.h2_version(), "bound_n": BOUND_N, "configs": []}
    failures = []
    for circuit, idx, k, recorded_sha in CONFIGS:
        if only and k not in only:
            continue
        params, first = setup(L, k)
        jsons = inputs(L, circuit, max(sizes))
        rows = []
        for n in sizes:
            r = Row(L, params, jsons[:n], idx, first)
            r.loop()                                                    # warm-up: key and params cached, blocks in the cache
            r.batch()
            loop_ms, spread, loops = timed(r.loop)
            batch_ms, batch_spread, batches = timed(r.batch)
            want = loops[0]
            if any(p != want for p in loops + batches):
                failures.append("%s k=%d n=%d: the two routes' proofs differ" % (circuit, k, n))
            if hashlib.sha256(batches[0][0]).hexdigest() != recorded_sha:
                failures.append("%s k=%d n=%d: item 0 is not the recorded proof" % (circuit, k, n))
            r.loop(False)
            r.batch(False)
            loop_os, _, _ = timed(lambda: r.loop(False))
            batch_os, _, _ = timed(lambda: r.batch(False))
            phases = traced(r.batch)
            row = {"n": n, "loop_ms": round(loop_ms, 3), "loop_spread_ms": round(spread, 3), "batch_ms": round(batch_ms, 3),
                   "batch_spread_ms": round(batch_spread, 3), "batch_over_loop": round(batch_ms / loop_ms, 4),
                   "per_proof_loop_ms": round(loop_ms / n, 4), "per_proof_batch_ms": round(batch_ms / n, 4),
                   "loop_os_ms": round(loop_os, 3), "batch_os_ms": round(batch_os, 3), "rng_calls_per_proof": r.streams.used(0),
                   "trace_ms": phases}
            rows.append(row)
            print(json.dumps({"circuit": circuit, "k": k, **row}), flush=True)
            if n == 1 and batch_ms > loop_ms + spread:
                failures.append("%s k=%d: a batch of one took %.3f ms, the single call %.3f ms (spread %.3f)"
                                % (circuit, k, batch_ms, loop_ms, spread))
            if n == BOUND_N and not batch_ms < loop_ms - spread:
                failures.append("%s k=%d: the batch of %d took %.3f ms, the loop %.3f ms (spread %.3f)"
                                % (circuit, k, n, batch_ms, loop_ms, spread))
        result["configs"].append({"circuit": circuit, "k": k, "proof_bytes": len(want[0]), "rows": rows})
    result["failures"] = failures
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("\n| circuit | k | N | loop ms | spread | batch ms | batch / loop | per proof: loop | batch | OS rng: loop | batch |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for cfg in result["configs"]:
        for row in cfg["rows"]:
            print("| %s | %d | %d | %.3f | %.3f | %.3f | %.2f | %.3f | %.3f | %.3f | %.3f |"
                  % (cfg["circuit"], cfg["k"], row["n"], row["loop_ms"], row["loop_spread_ms"], row["batch_ms"], row["batch_over_loop"],
                     row["per_proof_loop_ms"], row["per_proof_batch_ms"], row["loop_os_ms"], row["batch_os_ms"]))
    print("wrote " + args.out)
    for msg in failures:
        print("FAIL: " + msg, file=sys.stderr)
    return 1 if failures else 0


if __name__ == "__main__":
    sys.exit(main())
