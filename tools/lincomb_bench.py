"""h2_poly_lincomb_device timed against the public route it replaces, on the multiopen shapes of two proofs.

Shapes (BN254, random canonical columns, the circuits' own query lists from halo2_prover_amd/prover.py):
  * gwc_poseidon_k16      the GWC opening of the Poseidon proof at n = 2^16: one witness per distinct point
  * shplonk_collatz_k10   the SHPLONK opening of the Collatz proof at n = 2^10: h(X) and the final quotient
Two routes to the same columns, checked bit-equal before anything is timed:
  * call    opening.gwc_open / shplonk_open_h + shplonk_open_final: one h2_poly_lincomb_device call each
  * public  what a host had before: per term a copy of the column, h2_poly_scale_device and h2_poly_pointwise_device; per
            remainder a host upload and a subtraction; per point h2_poly_divide_linear_device
After --warmup rounds, --reps (>= 5) windows of --iters openings per route, the routes ALTERNATING window by window, each
window between two HIP events on the caller's stream: best, median and spread (max - min) in microseconds per opening.
`launches` counts what each route enqueues per opening (kernels and device copies), from the shapes.

--prover-parent FILE (a copy of an earlier halo2_prover_amd/prover.py) also times whole proofs of the Python prover,
Poseidon k = 11 and Collatz k = 10, this tree's against that file's: host wall clock around a proof that ends in a
device synchronise, alternating, --proof-reps each.

Prints one JSON document; --out FILE also writes it.  A measurement path: it needs the GPU and has no fallback.
"""
import argparse
import importlib.util
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
from halo2_prover_amd import opening, prover  # noqa: E402

P = prover.P


def random_columns(count, n, seed):
    import torch
    rng = np.random.default_rng(seed)
    host = rng.integers(0, 1 << 64, size=(count, n, 4), dtype=np.uint64)
    host[..., 3] = rng.integers(0, P >> 192, size=(count, n), dtype=np.uint64)          # canonical: below p
    return torch.from_numpy(host.view(np.int64)).cuda()


def query_list(circuit, k, seed):
    """create_proof's multiopen queries for `circuit` at n = 2^k over random columns: (point, column, key)"""
    n = 1 << k
    d, bf = circuit.degree, circuit.blinding_factors()
    dom = prover.EvaluationDomain(d, k, "bn254")
    omega = dom.omega
    nperm = len(circuit.permutation_columns)
    nz = (nperm + d - 3) // (d - 2)
    cols = random_columns(circuit.num_advice + circuit.num_fixed + nperm + nz + 2, n, seed)
    at = 0
    advice, at = cols[at:at + circuit.num_advice], at + circuit.num_advice
    fixed, at = cols[at:at + circuit.num_fixed], at + circuit.num_fixed
    sigma, at = cols[at:at + nperm], at + nperm
    z, at = cols[at:at + nz], at + nz
    h_poly, random_poly = cols[at], cols[at + 1]
    x = random.Random(seed).randrange(P)
    w_back = pow(omega, -(bf + 1), P)
    rot_point = lambda rot: x * pow(omega, rot, P) % P  # noqa: E731
    queries = [(rot_point(rot), advice[col], ("advice", col)) for col, rot in circuit.advice_queries]
    for i in range(nz):
        queries += [(x, z[i], ("z", i)), (x * omega % P, z[i], ("z", i))]
    for i in range(nz - 2, -1, -1):
        queries.append((x * w_back % P, z[i], ("z", i)))
    queries += [(rot_point(rot), fixed[col], ("fixed", col)) for col, rot in circuit.fixed_queries]
    queries += [(x, sigma[j], ("sigma", j)) for j in range(nperm)]
    queries += [(x, h_poly, ("h", 0)), (x, random_poly, ("random", 0))]
    return dom, queries


class PublicRoute:
    """the calls a host had before h2_poly_lincomb_device, as the Python prover made them; counts what it enqueues"""

    def __init__(self, dom):
        self.dom, self.launches = dom, 0
        self.dev = prover._Dev(dom, None)

    def scale(self, col, c):
        self.launches += 2                      # the copy, h2_poly_scale_device
        return self.dev.scale(col, c)

    def add_(self, a, b):
        self.launches += 1
        return self.dev.add_(a, b)

    def divide(self, col, points):
        import ctypes
        import torch
        q = col
        for pt in points:
            out = torch.empty_like(q)
            zm = self.dom.mont(pt)
            st = self.dom._L.h2_poly_divide_linear_device(self.dom.curve, ctypes.c_void_p(q.data_ptr()), q.shape[0], zm.ctypes.data,
                                                          ctypes.c_void_p(out.data_ptr()), self.dom._stream())
            assert st == 0
            self.launches += 3
            q = out
        return q

    def sub_low(self, col, low):
        # the upload, its conversion, the slice out, the subtraction, the slice back
        self.launches += 5
        k = len(low)
        col[:k] = self.dev.sub(col[:k].contiguous(), self.dev.from_ints(low))

    def gwc(self, queries, v):
        import torch
        points = []
        for pt, _, _ in queries:
            if pt not in points:
                points.append(pt)
        witnesses = []
        for pt in points:
            acc, vp = None, 1
            for qpt, col, _ in queries:
                if qpt == pt:
                    term = self.scale(col, vp)
                    acc = term if acc is None else self.add_(acc, term)
                    vp = vp * v % P
            witnesses.append(self.divide(acc, [pt]))
        self.launches += len(witnesses)         # the stack
        return torch.stack(witnesses)

    def shplonk(self, queries, evals, y, v, u):
        groups = opening.rotation_sets(queries)
        T = sorted({pt for pset, _ in groups for pt in pset})
        h, vp, per_set = None, 1, []
        for pset, members in groups:
            acc, yp, rems, rsum = None, 1, [], [0] * len(pset)
            for key, col in members:
                r = opening.interpolate(P, pset, [evals[(key, pt)] for pt in pset])
                rems.append(r)
                term = self.scale(col, yp)
                acc = term if acc is None else self.add_(acc, term)
                rsum = [(a + yp * b) % P for a, b in zip(rsum, r)]
                yp = yp * y % P
            self.sub_low(acc, rsum)
            term = self.scale(self.divide(acc, pset), vp)
            h = term if h is None else self.add_(h, term)
            vp = vp * v % P
            per_set.append((pset, members, rems))
        zt = 1
        for pt in T:
            zt = zt * (u - pt) % P
        Lc, vp, z0 = None, 1, None
        for pset, members, rems in per_set:
            z_i = 1
            for pt in T:
                if pt not in pset:
                    z_i = z_i * (u - pt) % P
            z0 = z_i if z0 is None else z0
            inner, yp, const = None, 1, 0
            for (key, col), r in zip(members, rems):
                term = self.scale(col, yp)
                inner = term if inner is None else self.add_(inner, term)
                const = (const + yp * prover._horner(r, u)) % P
                yp = yp * y % P
            self.sub_low(inner, [const])
            term = self.scale(inner, vp * z_i % P)
            Lc = term if Lc is None else self.add_(Lc, term)
            vp = vp * v % P
        self.launches += 2                      # the copy and the subtraction of L - zt h
        Lc = self.dev.sub(Lc, self.scale(h, zt))
        return h, self.scale(self.divide(Lc, [u]), pow(z0, -1, P))


def call_launches(jobs_points, extra_adds=0):
    """one h2_poly_lincomb_device call: the table upload, the sum, three scan kernels per round and eight jobs"""
    rounds = max(jobs_points) if jobs_points else 0
    scans = sum(3 * ((sum(1 for p in jobs_points if p > r) + 7) // 8) for r in range(rounds))
    return 2 + scans + extra_adds


def windows(routes, reps, iters, warmup):
    """routes: name -> callable; -> name -> microseconds per opening of every window, the routes alternating"""
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


def summary(ts):
    return {"best_us": round(min(ts), 1), "median_us": round(float(np.median(ts)), 1), "spread_us": round(max(ts) - min(ts), 1),
            "all_us": [round(t, 1) for t in ts]}


def bench_gwc(args):
    import torch
    dom, queries = query_list(prover.PoseidonCircuit([1, 2]), args.gwc_k, 11)
    v = random.Random(12).randrange(P)
    pub = PublicRoute(dom)
    want = pub.gwc(queries, v)
    launches_public = pub.launches
    got = opening.gwc_open(dom, queries, v)
    torch.cuda.synchronize()
    exact = bool(torch.equal(got, want))
    ts = windows({"call": lambda: opening.gwc_open(dom, queries, v), "public": lambda: pub.gwc(queries, v)},
                 args.reps, args.iters, args.warmup)
    return {"shape": "gwc_poseidon_k%d" % args.gwc_k, "n": 1 << args.gwc_k, "queries": len(queries), "witnesses": int(got.shape[0]),
            "exact": exact, "launches": {"call": call_launches([1] * int(got.shape[0])), "public": launches_public},
            "call": summary(ts["call"]), "public": summary(ts["public"])}


def bench_shplonk(args):
    import torch
    seq = [9, 28, 14, 7, 22, 11, 34, 17, 52, 26, 13, 40, 20, 10, 5, 16, 8, 4, 2, 1]
    dom, queries = query_list(prover.CollatzCircuit(seq), args.shplonk_k, 21)
    rng = random.Random(22)
    y, v, u = (rng.randrange(P) for _ in range(3))
    evals = {}
    for pt, col, key in queries:
        if (key, pt) not in evals:
            evals[(key, pt)] = dom.eval_polynomial(col.unsqueeze(0), pt)[0]
    pub = PublicRoute(dom)
    want_h, want_w = pub.shplonk(queries, evals, y, v, u)
    launches_public = pub.launches

    def call():
        h, state = opening.shplonk_open_h(dom, queries, evals, y, v)
        return h, opening.shplonk_open_final(state, u)
    got_h, got_w = call()
    torch.cuda.synchronize()
    exact = bool(torch.equal(got_h, want_h) and torch.equal(got_w, want_w))
    sets = [len(s) for s, _ in opening.rotation_sets(queries)]
    ts = windows({"call": call, "public": lambda: pub.shplonk(queries, evals, y, v, u)}, args.reps, args.iters, args.warmup)
    return {"shape": "shplonk_collatz_k%d" % args.shplonk_k, "n": 1 << args.shplonk_k, "queries": len(queries), "rotation_sets": sets,
            "exact": exact,
            "launches": {"call": call_launches(sets, extra_adds=len(sets) - 1) + call_launches([1]), "public": launches_public},
            "note": "both routes interpolate the remainders on the host inside the window",
            "call": summary(ts["call"]), "public": summary(ts["public"])}


def bench_proofs(args):
    """whole proofs of the Python prover: this tree's prover.py against the file given"""
    import torch
    spec = importlib.util.spec_from_file_location("halo2_prover_amd.prover_parent", args.prover_parent)
    parent = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = parent
    spec.loader.exec_module(parent)
    import pyref

    class Rng:
        def __init__(self, start):
            self.s = pyref.SurveyStream(start=start)

        def fill(self, n):
            return self.s.fill(n)

        def fr_random(self, _field=None):
            return self.s.fr_random(pyref.BN_FR)
    seq = [9, 28, 14, 7, 22, 11, 34, 17, 52, 26, 13, 40, 20, 10, 5, 16, 8, 4, 2, 1]
    rows = []
    for name, k, make, prove in (
            ("poseidon", 11, lambda m: m.PoseidonCircuit([1, 2]),
             lambda m, params, pk, c: m.generate_proof_with_instance(params, pk, c, [c.output()], Rng(8))),
            ("collatz", 10, lambda m: m.CollatzCircuit(seq), lambda m, params, pk, c: m.generate_proof(params, pk, c, Rng(8)))):
        params = prover.generate_params(k, Rng(0))
        made = {}
        for tag, m in (("this", prover), ("parent", parent)):
            c = make(m)
            made[tag] = (m, c, m.generate_keys(params, c))
        proofs = {tag: prove(m, params, pk, c) for tag, (m, c, pk) in made.items()}         # the warm-up, too
        times = {"this": [], "parent": []}
        for _ in range(args.proof_reps):
            for tag, (m, c, pk) in made.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                prove(m, params, pk, c)
                torch.cuda.synchronize()
                times[tag].append((time.perf_counter() - t0) * 1e3)
        rows.append({"circuit": name, "k": k, "same_bytes": proofs["this"] == proofs["parent"],
                     "this_ms": {"best": round(min(times["this"]), 1), "median": round(float(np.median(times["this"])), 1),
                                 "all": [round(t, 1) for t in times["this"]]},
                     "parent_ms": {"best": round(min(times["parent"]), 1), "median": round(float(np.median(times["parent"])), 1),
                                   "all": [round(t, 1) for t in times["parent"]]}})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--gwc-k", type=int, default=16)
    ap.add_argument("--shplonk-k", type=int, default=10)
    ap.add_argument("--prover-parent", default=None, help="an earlier halo2_prover_amd/prover.py to time whole proofs against")
    ap.add_argument("--proof-reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.reps >= 5 and args.iters >= 1
    h2.init(0)
    doc = {"tool": "tools/lincomb_bench.py", "timing": "HIP events around %d openings, per opening, routes alternating" % args.iters,
           "max_rounds": opening.max_rounds(), "openings": [bench_gwc(args), bench_shplonk(args)]}
    if args.prover_parent:
        doc["proofs"] = bench_proofs(args)
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    ok = all(r["exact"] for r in doc["openings"]) and all(r["same_bytes"] for r in doc.get("proofs", []))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
