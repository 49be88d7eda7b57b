"""h2_extended_to_coeff_device against the composed route it replaces: a clone of the extended columns,
h2_poly_mul_periodic_device (with t only), h2_ntt_scaled_device, h2_poly_coset_device over all 2^ext_k rows and the
contiguous copy of the kept prefix (what EvaluationDomain.divide_by_vanishing_poly + extended_to_coeff did before the
entry point existed; the clone stands for the fused call being out of place).  BN254; the domains are Poseidon's
(degree 6: extended_k = k + 3, out_len = 5 n): (k, columns) = (16, 1), (16, 7), (16, 16), (11, 7); each with and
without the t table.

Per shape: HIP events around each route on the caller's stream, twiddle tables and scratch warm, the two routes
ALTERNATED for --reps repetitions (>= 7); per route the best, the median and the spread (max - min), in milliseconds.
The results of the two routes are compared byte for byte before anything is timed.  Writes
profiles/extended_to_coeff_times.json (or --out FILE) and prints the table of DESIGN.md section 7.7.

Exits non-zero when the results differ, or when at extended_k = 19 the fused call is not faster than the composed route
by more than the composed route's own spread, at any column count.
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

DEGREE = 6
SHAPES = ((16, 1), (16, 7), (16, 16), (11, 7))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "extended_to_coeff_times.json"))
    args = ap.parse_args()
    assert args.reps >= 7
    import torch
    h2.init(0)
    L = h2lib.load()
    rows, ok = [], True
    for k, m in SHAPES:
        dom = EvaluationDomain(DEGREE, k, "bn254")
        ek, n = dom.extended_k, 1 << k
        en, hlen = 1 << ek, n * (DEGREE - 1)
        rng = np.random.default_rng(1000 * ek + m)
        host = rng.integers(0, 1 << 64, size=(m, en, 4), dtype=np.uint64)
        host[..., 3] = rng.integers(0, dom.p >> 192, size=(m, en), dtype=np.uint64)      # canonical: below p
        src = dom.to_device(host)
        work = torch.empty_like(src)
        wi, sc, zi = dom._m["extended_omega_inv"], dom._m["extended_ifft_divisor"], dom._m["g_coset_inv"]
        period = 1 << (ek - k)
        for with_t in (False, True):
            res = {}

            def fused():
                res["fused"] = dom.extended_to_coeff(src, divide_by_vanishing=with_t)

            def composed():
                work.copy_(src)
                p = ctypes.c_void_p(work.data_ptr())
                if with_t:
                    h2lib.check(L.h2_poly_mul_periodic_device(dom.curve, p, en, m, ctypes.c_void_p(dom.t_evaluations.data_ptr()),
                                                              period, dom._stream()), "h2_poly_mul_periodic_device")
                h2lib.check(L.h2_ntt_scaled_device(dom.curve, p, m, wi.ctypes.data, ek, sc.ctypes.data, dom._stream()),
                            "h2_ntt_scaled_device")
                h2lib.check(L.h2_poly_coset_device(dom.curve, p, en, m, zi.ctypes.data, dom._stream()), "h2_poly_coset_device")
                res["composed"] = work[:, :hlen, :].contiguous()

            for _ in range(2):                       # tables, scratch, allocator
                fused()
                composed()
            torch.cuda.synchronize()
            same = bool(torch.equal(res["fused"], res["composed"]))
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
            row = {"k": k, "ext_log_n": ek, "out_len": hlen, "columns": m, "t_table": with_t, "identical": same,
                   "reps": args.reps}
            for name, t in times.items():
                row[name] = {"best_ms": min(t), "median_ms": float(np.median(t)), "spread_ms": max(t) - min(t), "all_ms": t}
            row["gain_ms"] = row["composed"]["best_ms"] - row["fused"]["best_ms"]
            row["bar_met"] = row["gain_ms"] > row["composed"]["spread_ms"]
            if ek == 19:
                ok &= row["bar_met"]
            rows.append(row)
        del src, work
    print("| log ext | out_len | columns | t | composed best (spread) ms | fused best (spread) ms | gain ms | bar | identical |")
    print("|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        print("| %d | %d | %d | %s | %.3f (%.3f) | %.3f (%.3f) | %.3f | %s | %s |" % (
            r["ext_log_n"], r["out_len"], r["columns"], "yes" if r["t_table"] else "no", r["composed"]["best_ms"],
            r["composed"]["spread_ms"], r["fused"]["best_ms"], r["fused"]["spread_ms"], r["gain_ms"],
            "met" if r["bar_met"] else "MISSED", r["identical"]))
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/extended_to_coeff_bench.py", "curve": "bn254", "rows": rows}, f, indent=1)
        f.write("\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
