"""h2_poly_eval_device timed on (jobs, coefficients) grids over the three scalar fields.

Per field and shape: q random canonical columns of n coefficients resident in HBM, q random points; the result of one
call is checked against Python big-integer Horner on job 0 before anything is timed.  After --warmup calls (code
objects, the arena) a window of --iters calls sits between two HIP events on the caller's stream -- the whole call as a
host pays for it: the upload of the job table and the three launches -- and --reps (>= 5) windows give the best, the
median and the spread (max - min) in microseconds per call.  products = q (n + n / 16 + tiles) field products the
evaluation needs (runs, trees of 16-coefficient runs, fold; tiles of T = h2_poly_eval_tile()), over the best time.

Prints one JSON document; --out FILE also writes it.  A measurement path: it needs the GPU and has no fallback.
"""
import argparse
import ctypes
import json
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import halo2_prover_amd as h2  # noqa: E402
from halo2_prover_amd import lib as h2lib  # noqa: E402
from halo2_prover_amd.domain import _FIELDS  # noqa: E402

CURVES = (("bn254", 0), ("pallas", 1), ("vesta", 2))
SHAPES = ((32, 16), (1, 16), (8, 16), (128, 16), (32, 12), (8, 20), (4096, 6))       # (q, log2 n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--curves", default="bn254,pallas,vesta")
    ap.add_argument("--shapes", default=None, help="q:log2n,... (default: the built-in grid)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.reps >= 5 and args.iters >= 1
    shapes = SHAPES if not args.shapes else tuple(tuple(int(v) for v in s.split(":")) for s in args.shapes.split(","))
    import torch
    h2.init(0)
    L = h2lib.load()
    T = L.h2_poly_eval_tile()
    rows = []
    for name, cid in CURVES:
        if name not in args.curves.split(","):
            continue
        p = _FIELDS[cid][0]
        R = (1 << 256) % p
        for q, log_n in shapes:
            n = 1 << log_n
            rng = np.random.default_rng(1000 * log_n + q + cid)
            host = rng.integers(0, 1 << 64, size=(q, n, 4), dtype=np.uint64)
            host[..., 3] = rng.integers(0, p >> 192, size=(q, n), dtype=np.uint64)          # canonical: below p
            cols = torch.from_numpy(host.view(np.int64)).cuda()
            prng = random.Random(7 * log_n + q + cid)
            points = [prng.randrange(p) for _ in range(q)]
            pm = np.frombuffer(b"".join((x * R % p).to_bytes(32, "little") for x in points), dtype=np.uint64).copy()
            ptrs = (ctypes.c_void_p * q)(*[cols.data_ptr() + 32 * n * j for j in range(q)])
            out = torch.empty((q, 4), dtype=torch.int64, device="cuda")
            stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

            def run():
                h2lib.check(L.h2_poly_eval_device(cid, ptrs, n, pm.ctypes.data, q, ctypes.c_void_p(out.data_ptr()), stream),
                            "h2_poly_eval_device")

            for _ in range(args.warmup):
                run()
            torch.cuda.synchronize()
            got = int.from_bytes(out[0].cpu().numpy().tobytes(), "little")
            want = 0
            raw = host[0].tobytes()
            for i in range(n - 1, -1, -1):
                want = (want * points[0] + int.from_bytes(raw[32 * i:32 * i + 32], "little")) % p
            exact = got == want
            times = []
            for _ in range(args.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.iters):
                    run()
                e1.record()
                e1.synchronize()
                times.append(e0.elapsed_time(e1) * 1e3 / args.iters)
            tiles = (n + T - 1) // T
            products = q * (n + n // min(n, 16) + tiles)
            rows.append({"curve": name, "jobs": q, "log_n": log_n, "exact": exact, "reps": args.reps, "iters": args.iters,
                         "best_us": round(min(times), 2), "median_us": round(float(np.median(times)), 2),
                         "spread_us": round(max(times) - min(times), 2), "all_us": [round(t, 2) for t in times],
                         "products": products, "gproducts_per_s": round(products / (min(times) * 1e-6) / 1e9, 2)})
            del cols, out
    doc = {"tool": "tools/poly_eval_bench.py", "tile": T, "timing": "HIP events around %d calls, per call" % args.iters, "rows": rows}
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0 if all(r["exact"] for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
