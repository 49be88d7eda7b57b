"""h2_ipa_round_device timed round by round against the only route a host had for a round's MSMs before it.

Shapes: Pallas at k = 11 and k = 16, BN254 at k = 16 (--shapes curve:k,...); bases from the oracle's generator, registered
once as G || U || W; a random polynomial, fixed challenges and blinds.
  * new        h2_ipa_round_device: the fold, both expanded columns, both inner products, ONE two-column table MSM of
               n + 2 terms, the normalisation
  * yardstick  two h2_msm_points_device calls of `half` terms on the round's folded generators, uploaded in advance.  The
               generator fold and the inner products have no call there and are NOT charged: a lower bound for that route
Before anything is timed every round's L_j || R_j is compared with upstream's collapsing algorithm (generators folded by
the C oracle, the C oracle's best_multiexp), and the yardstick's two sums with the oracle's MSM over the folded generators.
After --warmup rounds, --reps (>= 5) windows of --iters calls per route and round, the routes ALTERNATING window by window,
each window between two HIP events on the stream the calls run on: best, median and spread (max - min) in microseconds
per round.  `opening` times begin + k rounds + final without the per-round read-back against the 2 k yardstick calls.
Bar (DESIGN.md section 7.5's rule): for every round with half >= 8 the new round's best is lower than the yardstick's best
by more than the yardstick's own spread; likewise the sums over the rounds.

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
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import halo2_prover_amd as h2  # noqa: E402
import oracle_lib as O  # noqa: E402
from halo2_prover_amd import lib as _lib  # noqa: E402
from halo2_prover_amd.transcript import FIELDS  # noqa: E402

CID = {"bn254": 0, "pallas": 1, "vesta": 2}


def limbs(values):
    buf = b"".join(int(v).to_bytes(32, "little") for v in values)
    return np.frombuffer(buf, dtype=np.uint64).reshape(-1, 4).copy()


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64).copy()).cuda()


def stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def jac_of(q, aff):
    aff = np.asarray(aff, dtype=np.uint64).reshape(-1, 8)
    out = np.zeros((aff.shape[0], 12), dtype=np.uint64)
    out[:, :8] = aff
    out[:, 8:] = limbs([(1 << 256) % q])[0]
    return out


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


def bench_shape(curve, k, args):
    import torch
    L = _lib.load()
    cid, n = CID[curve], 1 << k
    p, q, _ = FIELDS[cid]
    R = (1 << 256) % p
    mont = lambda vals: limbs([v % p * R % p for v in vals])  # noqa: E731
    rnd = random.Random(0xB0 + k + cid)
    pts = O.synth_bases(cid, 0x49504300 + 16 * k + cid, n + 2).reshape(n + 2, 8)
    bases = h2.Bases(curve, pts)
    a = [rnd.randrange(p) for _ in range(n)]
    x3, z = rnd.randrange(1, p), rnd.randrange(1, p)
    us = [rnd.randrange(1, p) for _ in range(k)]
    blinds = [(rnd.randrange(p), rnd.randrange(p)) for _ in range(k)]

    # upstream's collapsing algorithm: per round the folded generators, the two scalar halves and L_j || R_j
    A, B, G = a[:], [1] * n, pts[:n].copy()
    for i in range(1, n):
        B[i] = B[i - 1] * x3 % p
    want, yard_in = [], []
    for j in range(k):
        half = 1 << (k - j - 1)
        ipl = sum(x * y for x, y in zip(A[half:], B[:half])) % p
        ipr = sum(x * y for x, y in zip(A[:half], B[half:])) % p
        lr, plain = [], []
        for sc, gs, ip, bl in ((A[half:], G[:half], ipl, blinds[j][0]), (A[:half], G[half:], ipr, blinds[j][1])):
            tail = np.concatenate([gs, pts[n:]])
            lr.append(O.to_affine(cid, O.best_multiexp(cid, mont(list(sc) + [z * ip % p, bl]), tail, 8)))
            plain.append(O.to_affine(cid, O.best_multiexp(cid, mont(sc), gs, 8)))
        want.append(np.concatenate(lr))
        yard_in.append((to_dev(G[:half]), to_dev(G[half:]), to_dev(mont(A[half:])), to_dev(mont(A[:half])), half, plain))
        u, ui = us[j], pow(us[j], -1, p)
        A = [(A[i] + A[i + half] * ui) % p for i in range(half)]
        B = [(B[i] + B[i + half] * u) % p for i in range(half)]
        hi = O.scale_points(cid, mont([u])[0], jac_of(q, G[half:])).reshape(half, 12)
        lo = jac_of(q, G[:half])
        G = O.to_affine(cid, np.concatenate([O.jac_add(cid, lo[i], hi[i]) for i in range(half)])).reshape(half, 8)

    need = ctypes.c_size_t(0)
    assert L.h2_ipa_state_bytes(k, ctypes.byref(need)) == 0
    state = torch.empty(need.value // 8, dtype=torch.int64, device="cuda")
    out = torch.zeros(16, dtype=torch.int64, device="cuda")
    yout = torch.zeros(24, dtype=torch.int64, device="cuda")
    d_p = to_dev(mont(a))
    x3m, zm = mont([x3]), mont([z])
    um = [mont([u, pow(u, -1, p)]) for u in us]
    bm = [mont(bl) for bl in blinds]

    def begin():
        assert L.h2_ipa_begin_device(cid, k, ctypes.c_void_p(d_p.data_ptr()), x3m.ctypes.data, ctypes.c_void_p(state.data_ptr()),
                                     stream()) == 0

    def new_round(j):
        st = L.h2_ipa_round_device(cid, bases.handle, k, j, ctypes.c_void_p(state.data_ptr()),
                                   um[j - 1][0].ctypes.data if j else None, um[j - 1][1].ctypes.data if j else None,
                                   zm.ctypes.data, bm[j][0].ctypes.data, bm[j][1].ctypes.data, ctypes.c_void_p(out.data_ptr()),
                                   stream())
        assert st == 0

    def final():
        assert L.h2_ipa_final_device(cid, k, ctypes.c_void_p(state.data_ptr()), um[-1][0].ctypes.data, um[-1][1].ctypes.data,
                                     ctypes.c_void_p(out.data_ptr()), None, stream()) == 0

    def yard_round(j):
        g_lo, g_hi, a_hi, a_lo, half, _ = yard_in[j]
        for which, (g, s) in enumerate(((g_lo, a_hi), (g_hi, a_lo))):
            st = L.h2_msm_points_device(cid, ctypes.c_void_p(g.data_ptr()), ctypes.c_void_p(s.data_ptr()), half, half, 1,
                                        ctypes.c_void_p(yout.data_ptr() + 96 * which), stream())
            assert st == 0

    # both routes against the oracle before anything is timed
    exact, yard_exact = True, True
    begin()
    for j in range(k):
        new_round(j)
        exact = exact and np.array_equal(out.cpu().numpy().view(np.uint64), want[j])
        yard_round(j)
        got = O.to_affine(cid, yout.cpu().numpy().view(np.uint64))
        yard_exact = yard_exact and np.array_equal(got, np.concatenate(yard_in[j][5]))
    final()

    rows = []
    begin()
    for j in range(k):
        # round j reads generation j - 1, which the windows of round j - 1 left in place: it may be issued again and again
        ts = windows({"new": lambda: new_round(j), "yardstick": lambda: yard_round(j)}, args.reps, args.iters, args.warmup)
        new, yard = summary(ts["new"]), summary(ts["yardstick"])
        half = 1 << (k - j - 1)
        rows.append({"j": j, "half": half, "new": new, "yardstick": yard,
                     "bar": None if half < 8 else bool(new["best_us"] < yard["best_us"] - yard["spread_us"])})

    def opening():
        begin()
        for j in range(k):
            new_round(j)
        final()

    def yard_opening():
        for j in range(k):
            yard_round(j)
    ts = windows({"new": opening, "yardstick": yard_opening}, args.reps, max(1, args.iters // 4), 1)
    new, yard = summary(ts["new"]), summary(ts["yardstick"])
    bases.release()
    return {"curve": curve, "k": k, "exact": bool(exact), "yardstick_exact": bool(yard_exact), "rounds": rows,
            "sum_of_rounds_us": {"new_best": round(sum(r["new"]["best_us"] for r in rows), 1),
                                 "yardstick_best": round(sum(r["yardstick"]["best_us"] for r in rows), 1),
                                 "yardstick_spread": round(sum(r["yardstick"]["spread_us"] for r in rows), 1)},
            "opening": {"new": new, "yardstick": yard, "bar": bool(new["best_us"] < yard["best_us"] - yard["spread_us"])},
            "bar_rounds_met": all(r["bar"] for r in rows if r["bar"] is not None)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="pallas:11,pallas:16,bn254:16")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.reps >= 5 and args.iters >= 1
    h2.init(0)
    shapes = [(s.split(":")[0], int(s.split(":")[1])) for s in args.shapes.split(",")]
    doc = {"tool": "tools/ipa_bench.py",
           "timing": "HIP events around %d calls per window, per round, routes alternating, %d windows" % (args.iters, args.reps),
           "shapes": [bench_shape(c, k, args) for c, k in shapes]}
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0 if all(s["exact"] and s["yardstick_exact"] for s in doc["shapes"]) else 1


if __name__ == "__main__":
    sys.exit(main())
