"""h2_coeff_to_extended_device against the composed route it replaces: memset of the padded columns + copy of the n
coefficients + h2_poly_coset_device + h2_ntt_device (what EvaluationDomain.coeff_to_extended did before the entry
point existed).  BN254; shapes (log n, log extended n, columns): (16, 19, 7), (16, 19, 112), (11, 14, 7).

Per shape: HIP events around each route on the library's stream, twiddle tables and scratch warm, the two routes
ALTERNATED for --reps repetitions (>= 5); per route the best, the median and the spread (max - min), in milliseconds.
The results of the two routes are compared byte for byte before anything is timed.  Writes
profiles/coeff_to_extended_times.json (or --out FILE) and prints the table of DESIGN.md section 7.

Exits non-zero when the results differ, or when at (16, 19) the fused call is not faster than the composed route by
more than the composed route's own spread.
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import halo2_prover_amd as h2  # noqa: E402
from halo2_prover_amd import lib as h2lib  # noqa: E402
from halo2_prover_amd.domain import EvaluationDomain  # noqa: E402

SHAPES = ((16, 19, 7), (16, 19, 112), (11, 14, 7))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coeff_to_extended_times.json"))
    args = ap.parse_args()
    assert args.reps >= 5
    import torch
    h2.init(0)
    L = h2lib.load()
    rows, ok = [], True
    for k, ek, m in SHAPES:
        dom = EvaluationDomain((1 << (ek - k)) + 1, k, "bn254")       # j - 1 = 2^(ek - k): extended_k = ek
        assert dom.extended_k == ek
        n, en = 1 << k, 1 << ek
        rng = np.random.default_rng(1000 * ek + m)
        host = rng.integers(0, 1 << 64, size=(m, n, 4), dtype=np.uint64)
        host[..., 3] = rng.integers(0, dom.p >> 192, size=(m, n), dtype=np.uint64)      # canonical: below p
        src = dom.to_device(host)
        out_f = torch.empty((m, en, 4), dtype=torch.int64, device="cuda")
        out_c = torch.empty((m, en, 4), dtype=torch.int64, device="cuda")
        z, w = dom._m["g_coset"], dom._m["extended_omega"]

        def fused():
            h2lib.check(L.h2_coeff_to_extended_device(dom.curve, ctypes.c_void_p(src.data_ptr()), n, k, m, z.ctypes.data,
                                                      w.ctypes.data, ek, ctypes.c_void_p(out_f.data_ptr()), dom._stream()),
                        "h2_coeff_to_extended_device")

        def composed():
            out_c.zero_()
            out_c[:, :n, :] = src
            p = ctypes.c_void_p(out_c.data_ptr())
            h2lib.check(L.h2_poly_coset_device(dom.curve, p, en, m, z.ctypes.data, dom._stream()), "h2_poly_coset_device")
            h2lib.check(L.h2_ntt_device(dom.curve, p, m, w.ctypes.data, ek, dom._stream()), "h2_ntt_device")

        for _ in range(2):                       # tables, scratch, allocator
            fused()
            composed()
        torch.cuda.synchronize()
        same = bool(torch.equal(out_f, out_c))
        ok &= same
        times = {"fused": [], "composed": []}
        for _ in range(args.reps):
            for name, fn in (("composed", composed), ("fused", fused)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                times[name].append(e0.elapsed_time(e1))
        row = {"log_n": k, "ext_log_n": ek, "columns": m, "identical": same, "reps": args.reps}
        for name, t in times.items():
            row[name] = {"best_ms": min(t), "median_ms": float(np.median(t)), "spread_ms": max(t) - min(t), "all_ms": t}
        row["gain_ms"] = row["composed"]["best_ms"] - row["fused"]["best_ms"]
        row["bar_met"] = row["gain_ms"] > row["composed"]["spread_ms"]
        if ek == 19:
            ok &= row["bar_met"]
        rows.append(row)
        del src, out_f, out_c
    print("| log n | log ext | columns | composed best (spread) ms | fused best (spread) ms | gain ms | identical |")
    print("|---|---|---|---|---|---|---|")
    for r in rows:
        print("| %d | %d | %d | %.3f (%.3f) | %.3f (%.3f) | %.3f | %s |" % (
            r["log_n"], r["ext_log_n"], r["columns"], r["composed"]["best_ms"], r["composed"]["spread_ms"],
            r["fused"]["best_ms"], r["fused"]["spread_ms"], r["gain_ms"], r["identical"]))
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/coeff_to_extended_bench.py", "curve": "bn254", "rows": rows}, f, indent=1)
        f.write("\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
