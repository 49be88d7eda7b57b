"""h2_verify_proofs against a loop of h2_verify_proof calls: Poseidon at k = 6 and k = 16, Collatz (SHPLONK) at k = 10,
N = 1, 8, 64 and 512 proofs.  Writes profiles/verify_batch_times.json (or --out FILE).

Per (circuit, N): milliseconds for the loop of N single calls (the baseline: that code is unchanged), for one batch call
(best of five after two warm-ups, key cached), the H2_TRACE phases of one more batch call, and the decompression kernel
alone on that batch's points, timed with HIP events.  Exits non-zero when the two routes disagree about any proof, or
when the batch of 64 takes more than half the loop's time: the pairing alone is 53 % of a single verification and is paid
once per batch, so a batch that is not under half has lost the point of the feature somewhere.
"""
import argparse
import ctypes
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

SIZES = (1, 8, 64, 512)
CONFIGS = (("poseidon", 2, 6), ("poseidon", 2, 16), ("collatz", 0, 10))
BOUND_N, BOUND = 64, 0.5


def setup(L, k):
    cap = 4 + 128 * (1 << k) + 256
    buf = ctypes.create_string_buffer(cap)
    n = ctypes.c_size_t(0)
    h2lib.check(L.h2_setup(k, None, None, buf, cap, ctypes.byref(n)), "h2_setup")
    return buf.raw[:n.value]


def prove(L, params, js, idx):
    out = ctypes.create_string_buffer(1 << 16)
    n = ctypes.c_size_t(0)
    h2lib.check(L.h2_generate_proof(params, len(params), js.encode(), idx, None, None, out, 1 << 16, ctypes.byref(n)), "prove")
    return out.raw[:n.value]


def inputs(L, circuit, count):
    """`count` JSON inputs: distinct Poseidon messages; Collatz orbits of at most 32 entries, cycled when they run out"""
    out = []
    if circuit == "poseidon":
        buf = ctypes.create_string_buffer(256)
        n = ctypes.c_size_t(0)
        for i in range(count):
            msg = (1000 + i, 7 * i + 3)
            h2lib.check(L.h2_simulate(('{"x":[%d,%d]}' % msg).encode(), 2, buf, 256, ctypes.byref(n)), "h2_simulate")
            out.append('{"x":[%d,%d],"output":"%s"}' % (msg[0], msg[1], buf.value.decode()))
        return out
    orbits, start = [], 2
    while len(orbits) < min(count, 128):
        start += 1
        seq = [start]
        while seq[-1] != 1:
            seq.append(seq[-1] // 2 if seq[-1] % 2 == 0 else 3 * seq[-1] + 1)
        if len(seq) <= 32:
            orbits.append('{"x":%s}' % str(seq).replace(" ", ""))
    return [orbits[i % len(orbits)] for i in range(count)]


class Batch:
    def __init__(self, params, items, idx):
        n = len(items)
        self.params, self.idx, self.n, self.items = params, idx, n, items
        self.proofs = (ctypes.c_char_p * n)(*[p for p, _ in items])
        self.lens = (ctypes.c_size_t * n)(*[len(p) for p, _ in items])
        self.jsons = (ctypes.c_char_p * n)(*[j.encode() for _, j in items])
        self.ok = (ctypes.c_int * n)()
        self.all_ok = ctypes.c_int(0)

    def run(self, L):
        h2lib.check(L.h2_verify_proofs(self.params, len(self.params), self.n, self.proofs, self.lens, self.jsons, self.idx,
                                       None, None, self.ok, ctypes.byref(self.all_ok)), "h2_verify_proofs")
        return list(self.ok)

    def loop(self, L):
        ok = ctypes.c_int(0)
        res = []
        for proof, js in self.items:
            h2lib.check(L.h2_verify_proof(self.params, len(self.params), proof, len(proof), js.encode(), self.idx,
                                          ctypes.byref(ok)), "h2_verify_proof")
            res.append(ok.value)
        return res


def timed(fn, repeats):
    best, res = None, None
    for _ in range(repeats):
        t = time.perf_counter()
        res = fn()
        dt = (time.perf_counter() - t) * 1e3
        best = dt if best is None or dt < best else best
    return best, res


def traced(fn):
    """fn() with H2_TRACE set and this process's stderr caught: ({phase: summed ms}, checks, points)"""
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
    phases, checks, points = {}, None, None
    for line in text.splitlines():
        m = re.match(r"\[h2 verify_proofs\] (.+?)\s+[0-9.]+ ms \(\+([0-9.]+)\)", line)
        if m:
            phases[m.group(1)] = round(phases.get(m.group(1), 0.0) + float(m.group(2)), 3)
        m = re.match(r"\[h2 verify_proofs\] checks (\d+) of \d+ proofs \(\d+ replayed, (\d+) points\)", line)
        if m:
            checks, points = int(m.group(1)), int(m.group(2))
    return phases, checks, points


def decompress_ms(L, n, seed_words):
    """the decompression kernel on n points (the given 32-byte words, cycled), HIP events, best of five after two warm-ups"""
    import torch
    data = b"".join(seed_words[i % len(seed_words)] for i in range(n))
    d_in = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    d_out = torch.empty(64 * n, dtype=torch.uint8, device="cuda")
    d_st = torch.empty(n, dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    best = None
    for it in range(7):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        h2lib.check(L.h2_points_decompress_device(0, d_in.data_ptr(), n, d_out.data_ptr(), d_st.data_ptr(), s.cuda_stream),
                    "h2_points_decompress_device")
        e1.record(s)
        s.synchronize()
        ms = e0.elapsed_time(e1)
        if it >= 2 and (best is None or ms < best):
            best = ms
    assert int(d_st.cpu().sum()) == 0, "the bench's points must all decompress"
    return round(best, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_batch_times.json"))
    ap.add_argument("--sizes", default=",".join(str(s) for s in SIZES))
    args = ap.parse_args()
    sizes = [int(s) for s in args.sizes.split(",")]
    h2.init(0)
    L = h2.load()
    import torch
    result = {"device": torch.cuda.get_device_name(0), "h2_version": L.h2_version(), "bound": {"n": BOUND_N, "batch_over_loop": BOUND},
              "configs": []}
    failures = []
    first_word = None
    for circuit, idx, k in CONFIGS:
        params = setup(L, k)
        items = [(prove(L, params, js, idx), js) for js in inputs(L, circuit, max(sizes))]
        if first_word is None:
            first_word = [p[:32] for p, _ in items[:64]]
        rows = []
        for n in sizes:
            b = Batch(params, items[:n], idx)
            Batch(params, items[:min(n, 8)], idx).loop(L)               # warm-up (key and params cached from here on)
            loop_ms, single = timed(lambda: b.loop(L), 3 if n <= 64 else 1)
            b.run(L)
            b.run(L)
            batch_ms, batch = timed(lambda: b.run(L), 5)
            phases, checks, points = traced(lambda: b.run(L))
            row = {"n": n, "loop_ms": round(loop_ms, 3), "batch_ms": round(batch_ms, 3), "batch_over_loop": round(batch_ms / loop_ms, 4),
                   "per_proof_loop_ms": round(loop_ms / n, 4), "per_proof_batch_ms": round(batch_ms / n, 4),
                   "trace_ms": phases, "checks": checks, "points": points,
                   "decompress_kernel_ms": decompress_ms(L, points, [p[:32] for p, _ in items[:n]]) if points else None}
            rows.append(row)
            print(json.dumps({"circuit": circuit, "k": k, **row}), flush=True)
            if single != batch or single != [1] * n:
                failures.append("%s k=%d n=%d: the two routes differ (%r vs %r)" % (circuit, k, n, single, batch))
            if n == BOUND_N and batch_ms > BOUND * loop_ms:
                failures.append("%s k=%d: the batch of %d took %.2f ms, more than half of the loop's %.2f ms"
                                % (circuit, k, n, batch_ms, loop_ms))
        result["configs"].append({"circuit": circuit, "k": k, "proof_bytes": len(items[0][0]), "rows": rows})
    result["decompress_kernel_ms_n1600"] = decompress_ms(L, 1600, first_word)
    result["failures"] = failures
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("decompress n=1600: %.4f ms; wrote %s" % (result["decompress_kernel_ms_n1600"], args.out))
    for msg in failures:
        print("FAIL: " + msg, file=sys.stderr)
    return 1 if failures else 0


if __name__ == "__main__":
    sys.exit(main())
