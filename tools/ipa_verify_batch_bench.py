"""ipa.verify_proofs against a loop of ipa.verify_proof calls, and the two kernels behind it alone.  Writes
profiles/ipa_verify_batch_times.json (or --out FILE).

* verify_proofs against N calls of verify_proof for N = 1, 16, 256 at k = 8 and k = 16 on Pallas: wall-clock milliseconds,
  best of five after two warm-ups.  ONE proof per k is repeated under N transcripts (a proof costs as much to check the
  N-th time as the first: nothing is cached between items); verify_proof is the single path as it always was.
* The decompression kernel alone, HIP events, at n = N (2k + 1) and at 2^16 points for the three curves: Pallas and Vesta
  through h2_pasta_points_decompress_device, BN254 through h2_points_decompress_device -- the yardstick for what the
  discrete logarithm adds to a single power.
* h2_ipa_challenge_products_sum_device at k = 16 for count = 1, 64, 1024, HIP events around the call (the table upload
  included), beside h2_ipa_challenge_products_device (ONE vector: k launches).
Exits non-zero when the two routes disagree about any proof.
"""
import argparse
import ctypes
import json
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import halo2_prover_amd as h2  # noqa: E402
import oracle_lib as O  # noqa: E402
from halo2_prover_amd import ipa  # noqa: E402
from halo2_prover_amd import lib as h2lib  # noqa: E402
from halo2_prover_amd.transcript import FIELDS, compress, sqrt_mod  # noqa: E402

SIZES = (1, 16, 256)
KS = (8, 16)
COUNTS = (1, 64, 1024)


def limbs(values):
    buf = b"".join(int(v).to_bytes(32, "little") for v in values)
    return np.frombuffer(buf, dtype=np.uint64).reshape(-1, 4).copy()


class Rng:
    def __init__(self, seed):
        self.r = random.Random(seed)

    def __call__(self, n):
        return self.r.getrandbits(8 * n).to_bytes(n, "little")


def timed(fn, repeats=5, warmups=2):
    for _ in range(warmups):
        fn()
    best, res = None, None
    for _ in range(repeats):
        t = time.perf_counter()
        res = fn()
        dt = (time.perf_counter() - t) * 1e3
        best = dt if best is None or dt < best else best
    return best, res


def event_ms(enqueue, repeats=5, warmups=2):
    """best HIP-event time of enqueue(raw stream handle)"""
    import torch
    s = torch.cuda.Stream()
    best = None
    with torch.cuda.stream(s):
        for it in range(warmups + repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            enqueue(s.cuda_stream)
            e1.record(s)
            s.synchronize()
            ms = e0.elapsed_time(e1)
            if it >= warmups and (best is None or ms < best):
                best = ms
    return round(best, 4)


def one_proof(k):
    cid, n = 1, 1 << k
    pts = O.synth_bases(cid, 0x49564300 + 16 * k + cid, n + 2).reshape(n + 2, 8)
    params = ipa.ParamsIPA("pallas", k, pts[:n], pts[n + 1], pts[n])
    p = params.p
    rnd = random.Random(0xBE7C4 + k)
    R = (1 << 256) % p
    poly = [rnd.randrange(p) for _ in range(n)]
    blind, x3 = rnd.randrange(p), rnd.randrange(1, p)
    poly_m = limbs([c * R % p for c in poly])
    v = params.domain.eval_polynomial(params.column(poly_m).reshape(1, n, 4), x3)[0]
    proof = ipa.create_proof(params, h2.Blake2bTranscript("pallas"), poly_m, blind, x3, Rng(k))
    return params, dict(P=params.commit(poly_m, blind), x3=x3, v=v, proof=proof)


def curve_points(cid, count, seed):
    """`count` compressed points of the curve in its own wire form"""
    _, q, b = FIELDS[cid]
    rnd = random.Random(seed)
    out = []
    while len(out) < count:
        x = rnd.randrange(q)
        y = sqrt_mod(x * x * x + b, q)
        if y is not None:
            out.append(compress(cid, (x, y)))
    return out


def decompress_ms(L, cid, n, words):
    import torch
    data = b"".join(words[i % len(words)] for i in range(n))
    d_in = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    d_out = torch.empty(64 * n, dtype=torch.uint8, device="cuda")
    d_st = torch.empty(n, dtype=torch.uint8, device="cuda")
    fn = L.h2_points_decompress_device if cid == 0 else L.h2_pasta_points_decompress_device
    ms = event_ms(lambda s: h2lib.check(fn(cid, d_in.data_ptr(), n, d_out.data_ptr(), d_st.data_ptr(), s), "decompress"))
    assert int(d_st.cpu().sum()) == 0, "the bench's points must all decompress"
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ipa_verify_batch_times.json"))
    ap.add_argument("--sizes", default=",".join(str(s) for s in SIZES))
    ap.add_argument("--ks", default=",".join(str(s) for s in KS))
    args = ap.parse_args()
    sizes, ks = [int(s) for s in args.sizes.split(",")], [int(s) for s in args.ks.split(",")]
    h2.init(0)
    L = h2.load()
    import torch
    result = {"device": torch.cuda.get_device_name(0), "h2_version": L.h2_version(),
              "note": "one proof per k repeated under N transcripts; loop = N calls of ipa.verify_proof (unchanged by the batch "
                      "verifier); wall-clock ms, best of five after two warm-ups; kernel times from HIP events",
              "verify": [], "decompress_kernel_ms": [], "challenge_products_sum_ms": []}
    failures = []
    words = {cid: curve_points(cid, 64, 0x77 + cid) for cid in (0, 1, 2)}
    for k in ks:
        params, e = one_proof(k)
        rows = []
        for n in sizes:
            def batch():
                stats = {}
                items = [(h2.Blake2bTranscript("pallas", e["proof"]), e["P"], e["x3"], e["v"]) for _ in range(n)]
                return ipa.verify_proofs(params, items, stats=stats), stats

            def loop():
                return [ipa.verify_proof(params, h2.Blake2bTranscript("pallas", e["proof"]), e["P"], e["x3"], e["v"]) for _ in range(n)]
            loop_ms, single = timed(loop, 5 if n <= 16 else 2, 2 if n <= 16 else 1)
            batch_ms, (got, stats) = timed(batch)
            row = {"k": k, "n": n, "loop_ms": round(loop_ms, 3), "batch_ms": round(batch_ms, 3),
                   "batch_over_loop": round(batch_ms / loop_ms, 4), "per_proof_loop_ms": round(loop_ms / n, 4),
                   "per_proof_batch_ms": round(batch_ms / n, 4), **stats}
            rows.append(row)
            print(json.dumps(row), flush=True)
            if got != single or got != [True] * n:
                failures.append("k=%d n=%d: the two routes differ" % (k, n))
            for cid in (0, 1, 2):
                pts = n * (2 * k + 1)
                result["decompress_kernel_ms"].append({"curve": cid, "n": pts, "ms": decompress_ms(L, cid, pts, words[cid])})
        wins = [r["n"] for r in rows if r["batch_ms"] < r["loop_ms"]]
        result["verify"].append({"k": k, "proof_bytes": len(e["proof"]), "rows": rows, "first_n_where_batch_wins": min(wins) if wins else None})
    for cid in (0, 1, 2):
        result["decompress_kernel_ms"].append({"curve": cid, "n": 1 << 16, "ms": decompress_ms(L, cid, 1 << 16, words[cid])})
    for row in result["decompress_kernel_ms"]:
        print(json.dumps(row), flush=True)
    k = 16
    p = FIELDS[1][0]
    rnd = random.Random(0x53554D)
    out = torch.empty((1 << k, 4), dtype=torch.int64, device="cuda")
    R = (1 << 256) % p
    for count in COUNTS:
        um = limbs([rnd.randrange(p) for _ in range(count * k)]).reshape(-1)
        im = limbs([rnd.randrange(p) for _ in range(count)]).reshape(-1)
        ms = event_ms(lambda s: h2lib.check(L.h2_ipa_challenge_products_sum_device(1, um.ctypes.data, im.ctypes.data, k, count,
                                                                                    out.data_ptr(), s), "sum"))
        one = event_ms(lambda s: h2lib.check(L.h2_ipa_challenge_products_device(1, um.ctypes.data, k, im.ctypes.data, out.data_ptr(), s),
                                             "products"))
        row = {"k": k, "count": count, "sum_ms": ms, "us_per_proof": round(1e3 * ms / count, 3), "single_vector_ms": one}
        result["challenge_products_sum_ms"].append(row)
        print(json.dumps(row), flush=True)
    result["failures"] = failures
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote %s" % args.out)
    for msg in failures:
        print("FAIL: " + msg, file=sys.stderr)
    return 1 if failures else 0


if __name__ == "__main__":
    sys.exit(main())
