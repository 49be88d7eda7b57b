"""h2_ipa_*_batch_device timed against the only route a host had for m openings before it: one after the other.

Shapes: Pallas at k = 11 and k = 16, BN254 at k = 16 (--shapes curve:k,...), each with m in --batches (1,2,4,8,16,32)
openings; bases from the oracle's generator, registered once as G || U || W; every opening has its own random polynomial,
x3, z, challenges and blinds.
  * yardstick  m single openings one after the other on one stream, each h2_ipa_begin_device + k x h2_ipa_round_device +
               h2_ipa_final_device on its own state
  * lockstep   ONE batch: h2_ipa_begin_batch_device + k x h2_ipa_round_batch_device (one MSM of 2 m columns a round) +
               h2_ipa_final_batch_device
Neither route reads anything back inside a window (the challenges are fixed in advance), so both are charged what the
device does.  Before anything is timed every L_j || R_j, c and b[0] of the batch is compared with the single-opening route.
After --warmup runs, --reps (>= 5) windows of --iters runs per route, the routes ALTERNATING window by window, each window
between two HIP events on the stream the calls run on: best, median and spread (max - min) in microseconds per run.
`round` times one h2_ipa_round_batch_device call (round k / 2) the same way: the per-round time against m shows where a
round leaves the latency floor of the table MSM.
Bar (DESIGN.md section 7.5's rule): for every shape with m >= 2 the lockstep best is lower than the yardstick's best by
more than the yardstick's own spread.  m = 1 is reported: it should lie inside the single route's spread.

--trace RUNS runs the lockstep route alone RUNS times and times nothing: the program to put behind
`rocprofv3 --kernel-trace --stats --`, in a run of its own.

Prints one JSON document; --out FILE also writes it.  A measurement path: it needs the GPU and has no fallback.
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import halo2_prover_amd as h2  # noqa: E402
import oracle_lib as O  # noqa: E402
from halo2_prover_amd import lib as _lib  # noqa: E402
from halo2_prover_amd.transcript import FIELDS  # noqa: E402

CID = {"bn254": 0, "pallas": 1, "vesta": 2}


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64).copy()).cuda()


def stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def summary(ts):
    return {"best_us": round(min(ts), 1), "median_us": round(float(np.median(ts)), 1), "spread_us": round(max(ts) - min(ts), 1),
            "all_us": [round(t, 1) for t in ts]}


def windows(routes, reps, iters, warmup):
    import torch
    for _ in range(warmup):
        for fn in routes.values():
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in routes}
    for _ in range(reps):
        for name, fn in routes.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / iters)
    return times


def canonical(rng, count):
    """`count` field elements as (count, 4) limbs: 252 random bits, below every modulus here, so canonical as they are"""
    a = rng.integers(0, 1 << 63, size=(count, 4), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(count, 4), dtype=np.uint64)
    a[:, 3] >>= np.uint64(4)
    return a


def inverses(p, limbs):
    """elementwise 1 / x of Montgomery limbs, as Montgomery limbs"""
    R = (1 << 256) % p
    out = []
    for row in limbs:
        x = int.from_bytes(row.tobytes(), "little") * pow(R, -1, p) % p
        out.append(np.frombuffer((pow(x, -1, p) * R % p).to_bytes(32, "little"), dtype=np.uint64))
    return np.stack(out)


def bench_batch(L, cid, k, m, handle, rng, args):
    import torch
    n = 1 << k
    p = FIELDS[cid][0]
    polys = [to_dev(canonical(rng, n)) for _ in range(m)]
    x3, z = canonical(rng, m), canonical(rng, m)
    u = [canonical(rng, m) | np.uint64(1) for _ in range(k)]            # nonzero
    ui = [inverses(p, x) for x in u]
    lb, rb = [canonical(rng, m) for _ in range(k)], [canonical(rng, m) for _ in range(k)]

    need = ctypes.c_size_t(0)
    assert L.h2_ipa_state_bytes(k, ctypes.byref(need)) == 0
    states = [torch.empty(need.value // 8, dtype=torch.int64, device="cuda") for _ in range(m)]
    assert L.h2_ipa_batch_state_bytes(k, m, ctypes.byref(need)) == 0
    bstate = torch.empty(need.value // 8, dtype=torch.int64, device="cuda")
    out1 = torch.zeros(16, dtype=torch.int64, device="cuda")
    outm = torch.zeros((m, 16), dtype=torch.int64, device="cuda")
    d_p = (ctypes.c_void_p * m)(*[t.data_ptr() for t in polys])
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def single(i, keep=None):
        assert L.h2_ipa_begin_device(cid, k, ptr(polys[i]), x3[i].ctypes.data, ptr(states[i]), stream()) == 0
        for j in range(k):
            assert L.h2_ipa_round_device(cid, handle, k, j, ptr(states[i]), u[j - 1][i].ctypes.data if j else None,
                                         ui[j - 1][i].ctypes.data if j else None, z[i].ctypes.data, lb[j][i].ctypes.data,
                                         rb[j][i].ctypes.data, ptr(out1), stream()) == 0
            if keep is not None:
                keep.append(out1.cpu().numpy().copy())
        assert L.h2_ipa_final_device(cid, k, ptr(states[i]), u[-1][i].ctypes.data, ui[-1][i].ctypes.data, ptr(out1), None,
                                     stream()) == 0
        if keep is not None:
            keep.append(out1[:8].cpu().numpy().copy())

    def batch_begin():
        assert L.h2_ipa_begin_batch_device(cid, k, m, d_p, x3.ctypes.data, ptr(bstate), stream()) == 0

    def batch_round(j):
        assert L.h2_ipa_round_batch_device(cid, handle, k, j, m, ptr(bstate), u[j - 1].ctypes.data if j else None,
                                           ui[j - 1].ctypes.data if j else None, z.ctypes.data, lb[j].ctypes.data,
                                           rb[j].ctypes.data, ptr(outm), stream()) == 0

    def batch_final():
        assert L.h2_ipa_final_batch_device(cid, k, m, ptr(bstate), u[-1].ctypes.data, ui[-1].ctypes.data, ptr(outm), stream()) == 0

    def batch(keep=None):
        batch_begin()
        for j in range(k):
            batch_round(j)
            if keep is not None:
                keep.append(outm.cpu().numpy().copy())
        batch_final()
        if keep is not None:
            keep.append(outm.reshape(-1)[:8 * m].cpu().numpy().reshape(m, 8).copy())

    def yardstick():
        for i in range(m):
            single(i)

    if args.trace:                                    # for a kernel trace: the lockstep route alone, nothing compared or timed
        for _ in range(args.trace):
            batch()
        torch.cuda.synchronize()
        return {"m": m, "traced_runs": args.trace, "exact": True, "bar": None}
    # every output of the batch against the single-opening route before anything is timed
    got = []
    batch(got)
    exact = True
    for i in range(m):
        want = []
        single(i, want)
        exact = exact and all(np.array_equal(got[j][i], want[j]) for j in range(k + 1))

    iters = max(1, args.iters // m)
    ts = windows({"lockstep": batch, "yardstick": yardstick}, args.reps, iters, args.warmup)
    new, yard = summary(ts["lockstep"]), summary(ts["yardstick"])
    # one round of the batch, in the middle of an opening (a round may be issued again: it reads generation j - 1)
    jm = k // 2
    batch_begin()
    for j in range(jm):
        batch_round(j)
    rt = summary(windows({"round": lambda: batch_round(jm)}, args.reps, max(2, args.iters), args.warmup)["round"])
    return {"m": m, "exact": bool(exact), "iters_per_window": iters, "lockstep": new, "yardstick": yard,
            "speedup_best": round(yard["best_us"] / new["best_us"], 2),
            "bar": None if m < 2 else bool(new["best_us"] < yard["best_us"] - yard["spread_us"]),
            "m1_inside_spread": bool(abs(new["best_us"] - yard["best_us"]) <= yard["spread_us"]) if m == 1 else None,
            "round": dict(rt, j=jm, per_opening_us=round(rt["best_us"] / m, 1))}


def bench_shape(curve, k, args):
    L = _lib.load()
    cid, n = CID[curve], 1 << k
    pts = O.synth_bases(cid, 0x49504300 + 16 * k + cid, n + 2).reshape(n + 2, 8)
    bases = h2.Bases(curve, pts)
    rng = np.random.default_rng(0xBA7C0 + 16 * k + cid)
    rows = [bench_batch(L, cid, k, m, bases.handle, rng, args) for m in args.batches]
    bases.release()
    return {"curve": curve, "k": k, "batches": rows, "exact": all(r["exact"] for r in rows),
            "bar_met": all(r["bar"] for r in rows if r["bar"] is not None)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="pallas:11,pallas:16,bn254:16")
    ap.add_argument("--batches", default="1,2,4,8,16,32")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--trace", type=int, default=0, help="run the lockstep route alone this many times (under rocprofv3)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.reps >= 5 and args.iters >= 1
    args.batches = [int(x) for x in args.batches.split(",")]
    h2.init(0)
    shapes = [(s.split(":")[0], int(s.split(":")[1])) for s in args.shapes.split(",")]
    doc = {"tool": "tools/ipa_batch_bench.py",
           "timing": "HIP events around a window of whole runs (iters_per_window each), routes alternating, %d windows" % args.reps,
           "shapes": [bench_shape(c, k, args) for c, k in shapes]}
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0 if all(s["exact"] for s in doc["shapes"]) else 1


if __name__ == "__main__":
    sys.exit(main())
