"""h2_msm_points_device against the routes a host had before it, and the two sweeps behind its constants.  BN254.

Default mode -- the table-free call against the parent's only route for bases that are not registered,
h2_bases_register_device + h2_msm_device + h2_bases_release on the same device buffers, at n = 2^10, 2^13, 2^16, 2^20
with m = 1 and m = 4, and (no bar) against h2_msm_device alone on an already registered table.
--crossover -- n = 8 ... 8192 in powers of two, each of the call's two routes forced through
h2_selftest_set_msm_points_small_max: MSM_POINTS_SMALL_MAX (csrc/h2_tune.hpp) is the smallest swept n from which the
bucket route's median is lower.
--sweep -- the window width c = 6 ... 11 at the four sizes, m = 1 and 4; needs a tuning build (H2_BUILD_TUNING=1,
csrc/h2_tune.hpp: H2_TUNE_POINTS_C), given with --lib.

Method: warm scratch, HIP events on the library's stream around the enqueued work plus the final synchronise, the
routes ALTERNATED for --reps repetitions (7); per route the best, the median and the spread (max - min), in
milliseconds.  The results of the routes are compared after affine normalisation before anything is timed.  The points
are [s^i]G made on the device (h2_srs_generate); the scalars are uniform below r.

Default mode exits non-zero when results differ or when, at 2^16 or 2^20, the new call's best is not lower than the
parent route's best by more than the parent route's own spread.
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

P = 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47      # bn254 Fq
R_ORDER = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
CURVE = 0
SIZE_MAX = ctypes.c_size_t(-1).value


def to_int(limbs):
    return sum(int(x) << (64 * i) for i, x in enumerate(limbs))


def normalise(jac):
    """Jacobian (12 Montgomery limbs) -> the affine point as two integers (Montgomery factor left in: it is the same
    for both routes), None for the identity"""
    x, y, z = to_int(jac[0:4]), to_int(jac[4:8]), to_int(jac[8:12])
    if z == 0:
        return None
    rinv = pow(1 << 256, -1, P)
    x, y, z = x * rinv % P, y * rinv % P, z * rinv % P
    zi = pow(z, -1, P)
    return (x * zi * zi % P, y * zi * zi * zi % P)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--crossover", action="store_true")
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--lib", help="another build of libh2hip.so (the tuning build for --sweep)")
    ap.add_argument("--logs", default="10,13,16,20")
    ap.add_argument("--out")
    args = ap.parse_args()
    assert args.reps >= 5
    if args.lib:
        h2lib.LIB_PATH = os.path.abspath(args.lib)
    import torch
    h2.init(0)
    L = h2lib.load()
    rng = np.random.default_rng(0x48324D53)

    def make_points(n):
        buf = torch.empty((n, 8), dtype=torch.int64, device="cuda")
        s = np.array([0x1234567, 0, 0, 0], dtype=np.uint64)              # any scalar: the points only have to be valid
        h2lib.check(L.h2_srs_generate(CURVE, s.ctypes.data, n, ctypes.c_void_p(buf.data_ptr()), None), "h2_srs_generate")
        torch.cuda.synchronize()
        return buf

    def make_scalars(n, m):
        a = rng.integers(0, 1 << 64, size=(m, n, 4), dtype=np.uint64)
        a[..., 3] = rng.integers(0, R_ORDER >> 192, size=(m, n), dtype=np.uint64)       # canonical: below r
        return torch.from_numpy(a.view(np.int64)).cuda()

    def timed(fns, reps):
        """fns: name -> callable that enqueues on the library's stream; alternated"""
        times = {k: [] for k in fns}
        for _ in range(reps):
            for name, fn in fns.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                times[name].append(e0.elapsed_time(e1))
        return {k: {"best_ms": min(t), "median_ms": float(np.median(t)), "spread_ms": max(t) - min(t), "all_ms": t}
                for k, t in times.items()}

    def points_call(d_p, d_s, n, m, out):
        h2lib.check(L.h2_msm_points_device(CURVE, ctypes.c_void_p(d_p.data_ptr()), ctypes.c_void_p(d_s.data_ptr()), n, n, m,
                                           ctypes.c_void_p(out.data_ptr()), None), "h2_msm_points_device")

    def results(out, m):
        torch.cuda.synchronize()
        return [normalise(r) for r in out.cpu().numpy().view(np.uint64)[:m]]

    logs = [int(x) for x in args.logs.split(",")]
    rows, ok = [], True
    if args.crossover:
        n_max = 8192
        d_p, d_s = make_points(n_max), make_scalars(n_max, 1)
        out_a = torch.zeros((1, 12), dtype=torch.int64, device="cuda")
        out_b = torch.zeros((1, 12), dtype=torch.int64, device="cuda")
        try:
            n = 8
            while n <= n_max:
                def small():
                    L.h2_selftest_set_msm_points_small_max(1 << 30)
                    points_call(d_p, d_s, n, 1, out_a)

                def buckets():
                    L.h2_selftest_set_msm_points_small_max(0)
                    points_call(d_p, d_s, n, 1, out_b)

                for _ in range(2):
                    small()
                    buckets()
                same = results(out_a, 1) == results(out_b, 1)
                ok &= same
                row = {"n": n, "identical": same}
                row.update(timed({"double_and_add": small, "buckets": buckets}, args.reps))
                rows.append(row)
                n *= 2
        finally:
            L.h2_selftest_set_msm_points_small_max(SIZE_MAX)
        print("| n | double-and-add median (best, spread) ms | buckets median (best, spread) ms | identical |")
        print("|---|---|---|---|")
        for r in rows:
            a, b = r["double_and_add"], r["buckets"]
            print("| %d | %.3f (%.3f, %.3f) | %.3f (%.3f, %.3f) | %s |" % (r["n"], a["median_ms"], a["best_ms"], a["spread_ms"],
                                                                         b["median_ms"], b["best_ms"], b["spread_ms"], r["identical"]))
        # the smallest swept n FROM WHICH the bucket route's median is lower (at it and at every larger swept n)
        cross = None
        for r in reversed(rows):
            if r["buckets"]["median_ms"] < r["double_and_add"]["median_ms"]:
                cross = r["n"]
            else:
                break
        print("crossover: %s" % cross)
        record = {"tool": "tools/msm_points_bench.py --crossover", "curve": "bn254", "reps": args.reps, "crossover": cross, "rows": rows}
    elif args.sweep:
        for lg in logs:
            n = 1 << lg
            d_p = make_points(n)
            for m in (1, 4):
                d_s = make_scalars(n, m)
                out = torch.zeros((m, 12), dtype=torch.int64, device="cuda")
                first = None
                for c in range(6, 12):
                    os.environ["H2_TUNE_POINTS_C"] = str(c)
                    plan = h2.msm_points_plan(n)
                    assert plan["window_bits"] in (c, c - 1), "not a tuning build: H2_TUNE_POINTS_C has no effect"

                    def call():
                        points_call(d_p, d_s, n, m, out)

                    for _ in range(2):
                        call()
                    res = results(out, m)
                    first = first or res
                    ok &= res == first
                    row = {"log_n": lg, "columns": m, "c_asked": c, "window_bits": plan["window_bits"], "windows": plan["windows"],
                           "identical": res == first}
                    row.update(timed({"points": call}, args.reps))
                    rows.append(row)
                del d_s, out
            del d_p
        os.environ.pop("H2_TUNE_POINTS_C", None)
        print("| log n | columns | c | windows | median (best, spread) ms |")
        print("|---|---|---|---|---|")
        for r in rows:
            t = r["points"]
            print("| %d | %d | %d | %d | %.3f (%.3f, %.3f) |" % (r["log_n"], r["columns"], r["window_bits"], r["windows"], t["median_ms"],
                                                              t["best_ms"], t["spread_ms"]))
        record = {"tool": "tools/msm_points_bench.py --sweep", "curve": "bn254", "reps": args.reps, "rows": rows}
    else:
        for lg in logs:
            n = 1 << lg
            d_p = make_points(n)
            for m in (1, 4):
                d_s = make_scalars(n, m)
                out_new = torch.zeros((m, 12), dtype=torch.int64, device="cuda")
                out_old = torch.zeros((m, 12), dtype=torch.int64, device="cuda")
                out_reg = torch.zeros((m, 12), dtype=torch.int64, device="cuda")
                resident = h2.Bases.from_device(CURVE, d_p.data_ptr(), n)

                def new():
                    points_call(d_p, d_s, n, m, out_new)

                def parent_route():
                    hnd = ctypes.c_uint64(0)
                    h2lib.check(L.h2_bases_register_device(CURVE, ctypes.c_void_p(d_p.data_ptr()), n, ctypes.byref(hnd)), "register")
                    h2lib.check(L.h2_msm_device(CURVE, hnd.value, ctypes.c_void_p(d_s.data_ptr()), n, m,
                                                ctypes.c_void_p(out_old.data_ptr()), None), "h2_msm_device")
                    h2lib.check(L.h2_bases_release(hnd.value), "release")

                def registered():
                    resident.msm_device(d_s.data_ptr(), n, m, out_reg.data_ptr())

                for _ in range(2):
                    new()
                    parent_route()
                    registered()
                a, b, c = results(out_new, m), results(out_old, m), results(out_reg, m)
                same = a == b == c
                ok &= same
                plan = h2.msm_points_plan(n)
                row = {"log_n": lg, "columns": m, "identical": same, "route": plan["route"], "window_bits": plan["window_bits"],
                       "windows": plan["windows"], "reps": args.reps}
                row.update(timed({"parent_route": parent_route, "points": new, "registered": registered}, args.reps))
                row["gain_ms"] = row["parent_route"]["best_ms"] - row["points"]["best_ms"]
                row["bar"] = lg in (16, 20)
                row["bar_met"] = row["gain_ms"] > row["parent_route"]["spread_ms"]
                row["ratio_to_registered"] = row["points"]["best_ms"] / row["registered"]["best_ms"]
                if row["bar"]:
                    ok &= row["bar_met"]
                rows.append(row)
                resident.release()
                del d_s, out_new, out_old, out_reg
            del d_p
        print("| log n | columns | register + msm + release best / median (spread) ms | h2_msm_points best / median (spread) ms | gain ms | bar | "
              "registered table alone best ms | ratio | identical |")
        print("|---|---|---|---|---|---|---|---|---|")
        for r in rows:
            o, p, g = r["parent_route"], r["points"], r["registered"]
            print("| %d | %d | %.3f / %.3f (%.3f) | %.3f / %.3f (%.3f) | %.3f | %s | %.3f | %.2f | %s |" % (
                r["log_n"], r["columns"], o["best_ms"], o["median_ms"], o["spread_ms"], p["best_ms"], p["median_ms"], p["spread_ms"],
                r["gain_ms"], ("met" if r["bar_met"] else "MISSED") if r["bar"] else "-", g["best_ms"], r["ratio_to_registered"],
                r["identical"]))
        record = {"tool": "tools/msm_points_bench.py", "curve": "bn254", "rows": rows}
    if args.out:
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
