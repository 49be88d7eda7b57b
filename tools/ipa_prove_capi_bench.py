"""ipa.create_proofs_bytes (ONE h2_ipa_create_proofs call: the transcripts on the device, no read-back between rounds)
against ipa.create_proofs (the host loop, the yardstick), and the transcript step's two inversions.  Writes
profiles/ipa_prove_capi_times.json (or --out FILE).

* Both routes on the same m openings for m = 1, 4, 32 at k = 11 and k = 16 on Pallas: the polynomials are expanded on the
  device from seeds, s_poly comes from each item's 32-byte seed on both routes, and the bytes of the two routes are compared
  BEFORE anything is timed.  Then the routes alternate, five windows each after one warm-up each; a window is `calls` calls
  and ends in the route's own last synchronisation, wall-clock milliseconds per call.  Reported: best, median, spread
  (largest minus smallest window).  The bar (DESIGN.md section 7.5's rule): the new route's best is below the yardstick's
  best by more than the yardstick's own spread.  Making the items (transcripts, rngs) is inside the timed region of both.
* h2_ipa_prove_rounds_device alone at k = 11, HIP events, with the step kernel inverting by divsteps and by fe_inv's Fermat
  chain: the difference over the k step launches that invert is what one inversion form costs more than the other.  The
  kernel's own time per launch comes from a trace (rocprofv3 --kernel-trace --stats on `--workload`, a run of its own; the
  two forms are two template instances, so the trace names them apart); `--merge-trace CSV` adds its rows to the file.
Exits non-zero when the two routes disagree about any proof.
"""
import argparse
import csv
import ctypes
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import halo2_prover_amd as h2  # noqa: E402
import oracle_lib as O  # noqa: E402
from halo2_prover_amd import ipa  # noqa: E402
from halo2_prover_amd import lib as h2lib  # noqa: E402

KS = (11, 16)
MS = (1, 4, 32)
WINDOWS = 5
CURVE, CID = "pallas", 1


class Rng:
    def __init__(self, seed):
        self.r = random.Random(seed)

    def __call__(self, n):
        return self.r.getrandbits(8 * n).to_bytes(n, "little")


def setup(k):
    n = 1 << k
    pts = O.synth_bases(CID, 0x49505600 + 16 * k + CID, n + 2).reshape(n + 2, 8)
    return ipa.ParamsIPA(CURVE, k, pts[:n], pts[n + 1], pts[n])


def openings(params, m, seed):
    """m polynomials expanded on the device, their blinds and points"""
    import torch
    L, n, p = params._L, params.n, params.p
    rnd = random.Random(seed)
    out = []
    for i in range(m):
        poly = torch.empty((n, 4), dtype=torch.int64, device="cuda")
        key = bytes(rnd.getrandbits(8) for _ in range(32))
        h2lib.check(L.h2_chacha20_scalars_device(CID, key, 0, n, ctypes.c_void_p(poly.data_ptr()), None), "chacha")
        out.append(dict(poly=poly, blind=rnd.randrange(p), x3=rnd.randrange(1, p), rng=seed * 1000 + i))
    torch.cuda.synchronize()
    return out


def host_route(params, S, prefix):
    items = []
    for s in S:
        tr = h2.Blake2bTranscript(CURVE)
        tr.state.update(prefix)
        items.append((tr, s["poly"], s["blind"], s["x3"], Rng(s["rng"]), None))
    return ipa.create_proofs(params, items)


def capi_route(params, S, prefix):
    items = []
    for s in S:
        mid = h2.Blake2bMidstate(CURVE)
        mid.update(prefix)
        items.append((mid, s["poly"], s["blind"], s["x3"], Rng(s["rng"]), None))
    return ipa.create_proofs_bytes(params, items)


def window(fn, calls):
    t = time.perf_counter()
    for _ in range(calls):
        fn()
    return (time.perf_counter() - t) * 1e3 / calls


def summary(ws):
    return {"best_ms": round(min(ws), 4), "median_ms": round(statistics.median(ws), 4), "spread_ms": round(max(ws) - min(ws), 4),
            "windows_ms": [round(w, 4) for w in ws]}


def rounds_ms(params, S, form):
    """h2_ipa_prove_rounds_device alone (HIP events, best of five after two warm-ups) with the step inverting by `form`"""
    import torch
    L, k, p, m = params._L, params.k, params.p, len(S)
    need = ctypes.c_size_t(0)
    h2lib.check(L.h2_ipa_prove_state_bytes(k, m, ctypes.byref(need)), "state bytes")
    state = torch.empty(need.value // 8, dtype=torch.int64, device="cuda")
    tail = torch.empty(m * (2 * k + 2) * 4, dtype=torch.int64, device="cuda")
    status = torch.empty(m, dtype=torch.int32, device="cuda")
    rnd = random.Random(0x0DD5)
    import numpy as np
    sc = lambda cnt: np.ascontiguousarray(np.concatenate([params.mont(rnd.randrange(p)) for _ in range(cnt)]))  # noqa: E731
    x3, z, f0, blinds = sc(m), sc(m), sc(m), sc(2 * k * m)
    states = ctypes.create_string_buffer(h2.Blake2bMidstate(CURVE).export() * m, 208 * m)
    d_p = (ctypes.c_void_p * m)(*[s["poly"].data_ptr() for s in S])
    h2lib.check(L.h2_selftest_set_ipa_inv_form(form), "form")
    s = torch.cuda.Stream()
    best = None
    try:
        with torch.cuda.stream(s):
            for it in range(7):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s)
                h2lib.check(L.h2_ipa_prove_rounds_device(CID, params.bases.handle, k, m, d_p, x3.ctypes.data, z.ctypes.data, f0.ctypes.data,
                                                         blinds.ctypes.data, states, ctypes.c_void_p(state.data_ptr()),
                                                         ctypes.c_void_p(tail.data_ptr()), None, ctypes.c_void_p(status.data_ptr()),
                                                         ctypes.c_void_p(s.cuda_stream)), "rounds")
                e1.record(s)
                s.synchronize()
                ms = e0.elapsed_time(e1)
                if it >= 2 and (best is None or ms < best):
                    best = ms
    finally:
        h2lib.check(L.h2_selftest_set_ipa_inv_form(0), "form")
    assert not status.cpu().any()
    return round(best, 4)


def merge_trace(path, out):
    """the step kernel's rows of a rocprofv3 kernel-stats CSV -> the result file"""
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            name = r.get("Name") or r.get("KernelName") or ""
            if "ipa_prove_step_kernel" in name:
                form = "fermat" if ", 1>" in name or ",1>" in name else "divsteps"
                rows.append({"inversion": form, "calls": int(r["Calls"]), "average_us": round(float(r["AverageNs"]) / 1e3, 3),
                             "min_us": round(float(r["MinNs"]) / 1e3, 3), "max_us": round(float(r["MaxNs"]) / 1e3, 3)})
    with open(out) as f:
        result = json.load(f)
    result["step_kernel_trace"] = rows
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(rows))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ipa_prove_capi_times.json"))
    ap.add_argument("--ks", default=",".join(str(s) for s in KS))
    ap.add_argument("--ms", default=",".join(str(s) for s in MS))
    ap.add_argument("--workload", action="store_true", help="for a profiler: a few calls at k = 11, m = 1 and 4, each inversion form")
    ap.add_argument("--merge-trace", default=None, help="a rocprofv3 kernel_stats.csv whose step-kernel rows go into --out")
    args = ap.parse_args()
    if args.merge_trace:
        merge_trace(args.merge_trace, args.out)
        return 0
    ks, ms = [int(s) for s in args.ks.split(",")], [int(s) for s in args.ms.split(",")]
    h2.init(0)
    L = h2.load()
    import torch
    prefix = bytes(random.Random(0x50524658).getrandbits(8) for _ in range(100))
    if args.workload:
        params = setup(11)
        for m in (1, 4):
            S = openings(params, m, 0xBE00 + m)
            for form in (0, 1):
                h2lib.check(L.h2_selftest_set_ipa_inv_form(form), "form")
                for _ in range(3):
                    capi_route(params, S, prefix)
        h2lib.check(L.h2_selftest_set_ipa_inv_form(0), "form")
        return 0
    result = {"device": torch.cuda.get_device_name(0), "h2_version": L.h2_version(), "curve": CURVE,
              "note": "host = ipa.create_proofs (the host loop: k read-backs, unchanged by this route), capi = ipa.create_proofs_bytes "
                      "(one h2_ipa_create_proofs call); same openings, s_poly from each item's seed on both; bytes compared before "
                      "timing; routes alternate, %d windows each, wall-clock ms per call, making the items included; spread = largest "
                      "minus smallest window; bar: capi best < host best - host spread" % WINDOWS,
              "create_proofs": [], "rounds_call_ms": []}
    failures = []
    for k in ks:
        params = setup(k)
        calls = 4 if k <= 12 else 2
        for m in ms:
            S = openings(params, m, 0xBE00 + 64 * k + m)
            want, got = host_route(params, S, prefix), capi_route(params, S, prefix)
            if want != got:
                failures.append("k=%d m=%d: the two routes' bytes differ" % (k, m))
                continue
            host_route(params, S, prefix)
            capi_route(params, S, prefix)
            hw, cw = [], []
            for _ in range(WINDOWS):
                hw.append(window(lambda: host_route(params, S, prefix), calls))
                cw.append(window(lambda: capi_route(params, S, prefix), calls))
            hs, cs = summary(hw), summary(cw)
            row = {"k": k, "m": m, "calls_per_window": calls, "host": hs, "capi": cs,
                   "capi_over_host_best": round(cs["best_ms"] / hs["best_ms"], 4),
                   "saved_per_round_us": round(1e3 * (hs["best_ms"] - cs["best_ms"]) / k, 2),
                   "bar_met": cs["best_ms"] < hs["best_ms"] - hs["spread_ms"]}
            result["create_proofs"].append(row)
            print(json.dumps(row), flush=True)
            if k == ks[0]:
                t0, t1 = rounds_ms(params, S, 0), rounds_ms(params, S, 1)
                rrow = {"k": k, "m": m, "divsteps_ms": t0, "fermat_ms": t1, "fermat_minus_divsteps_per_step_us": round(1e3 * (t1 - t0) / k, 2)}
                result["rounds_call_ms"].append(rrow)
                print(json.dumps(rrow), flush=True)
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
