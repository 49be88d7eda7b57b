"""h2_poseidon_hash_device and h2_poseidon_merkle_device timed against the in-run modmul ceiling.

Per scalar field (BN254 (8, 60), Pallas and Vesta (8, 56)):
  * hash        ConstantLength<2> of n = 2^10 .. 2^22 messages: ns per hash, and field products per second -- 18 r_f + 12 r_p
                per permutation in the plain form, 864 and 816 -- as a fraction of h2_selftest_modmul_rate taken in the same
                run at four waves per SIMD.  That hook times the BASE field of a curve: Pallas's scalar field is Vesta's
                base field and the other way round, so the Pasta fractions are like for like; BN254's Fr is held against
                Fq, the other dense 254-bit modulus (the same instruction count, not the same constants).
  * merkle      a tree of 2^20 leaves, one call.
  * tail sweep  the same call at depth 12 and 20 with the tail width T = 1 (a launch per level), 32 .. 512
                (h2_selftest_set_poseidon_merkle_tail), the settings alternating window by window.
  * product     the hash kernel on the compiler's form of the product against the single-chain form of
                csrc/h2_field29_chain.hpp (h2_selftest_set_poseidon_form 1 / 2; Pasta fields only) at n = 2^12 .. 2^20,
                alternating.  Everything else runs with the choice by size in force (form 0).
Before anything is timed the first hashes of each field are compared with the host's big-integer hash.  After --warmup
calls, --reps windows of --iters calls between two HIP events on the stream the calls run on: best, median and spread.

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
import halo2_prover_amd as h2  # noqa: E402
from halo2_prover_amd import lib as _lib  # noqa: E402
from halo2_prover_amd import poseidon  # noqa: E402

NAMES = {0: "bn254", 1: "pallas", 2: "vesta"}
RATE_CURVE = {0: 0, 1: 2, 2: 1}          # the curve whose BASE field stands for this curve's scalar field


def stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def elements(n, seed):
    """n canonical field elements on the device: random limbs below 2^253"""
    import torch
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    a = torch.randint(-(1 << 62), 1 << 62, (n, 4), dtype=torch.int64, device="cuda", generator=g)
    a[:, 3] &= (1 << 61) - 1
    return a


def summary(ts):
    return {"best_us": round(min(ts), 2), "median_us": round(float(np.median(ts)), 2), "spread_us": round(max(ts) - min(ts), 2)}


def windows(routes, reps, iters, warmup):
    """routes: name -> (prepare, call); `prepare` runs outside the timed window"""
    import torch
    for prepare, fn in routes.values():
        prepare()
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in routes}
    for _ in range(reps):
        for name, (prepare, fn) in routes.items():
            prepare()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / iters)
    return {name: summary(ts) for name, ts in times.items()}


def bench_field(cid, args):
    import torch
    L = _lib.load()
    r_f, r_p = poseidon.DEFAULT_ROUNDS[cid]
    products = 18 * r_f + 12 * r_p
    rate = ctypes.c_double(0)
    _lib.check(L.h2_selftest_modmul_rate(RATE_CURVE[cid], 4, 4096, ctypes.byref(rate)), "h2_selftest_modmul_rate")
    nmax = 1 << args.max_log_n
    msgs = elements(2 * nmax, 0x9051 + cid)
    out = torch.empty((nmax, 4), dtype=torch.int64, device="cuda")

    def hash_call(n):
        st = L.h2_poseidon_hash_device(cid, r_f, r_p, ctypes.c_void_p(msgs.data_ptr()), 2, 2, n, ctypes.c_void_p(out.data_ptr()), stream())
        assert st == 0

    def nothing():
        pass

    hash_call(8)
    got = poseidon.from_mont(cid, out[:8].cpu().numpy().view(np.uint64))
    m = poseidon.from_mont(cid, msgs[:16].cpu().numpy().view(np.uint64))
    exact = got == [poseidon.hash2_int(cid, m[2 * i], m[2 * i + 1]) for i in range(8)]

    rows = []
    for log_n in range(10, args.max_log_n + 1):
        n = 1 << log_n
        t = windows({"hash": (nothing, lambda: hash_call(n))}, args.reps, max(1, min(args.iters, (1 << 22) >> log_n)), args.warmup)["hash"]
        rows.append({"log_n": log_n, **t, "ns_per_hash": round(t["best_us"] * 1e3 / n, 3),
                     "products_per_s": round(n * products / (t["best_us"] * 1e-6), 0),
                     "fraction_of_modmul_rate": round(n * products / (t["best_us"] * 1e-6) / rate.value, 4)})

    def merkle_call(depth):
        st = L.h2_poseidon_merkle_device(cid, r_f, r_p, ctypes.c_void_p(msgs.data_ptr()), depth, ctypes.c_void_p(out.data_ptr()), stream())
        assert st == 0

    def tail(t):
        return lambda: _lib.check(L.h2_selftest_set_poseidon_merkle_tail(t), "set tail")

    tree_log = min(20, args.max_log_n)
    merkle = windows({"merkle": (tail(0), lambda: merkle_call(tree_log))}, args.reps, 2, 1)["merkle"]
    sweep = {}
    for depth in (12, tree_log):
        routes = {"T=%d" % t: (tail(t), (lambda d: lambda: merkle_call(d))(depth)) for t in (1, 32, 64, 128, 256, 512)}
        sweep["depth_%d" % depth] = windows(routes, args.reps + 2, 4 if depth == 12 else 2, 1)
    tail(0)()

    product = None
    if cid != 0:
        def form(which):
            return lambda: _lib.check(L.h2_selftest_set_poseidon_form(which), "set form")
        product = {}
        for log_n in sorted({12, 15, 16, 17, 18, min(20, args.max_log_n)}):
            n = 1 << log_n
            product["log_n_%d" % log_n] = windows({"compiler": (form(1), lambda: hash_call(n)), "chain": (form(2), lambda: hash_call(n))},
                                                  args.reps, 4, args.warmup)
        form(0)()
    return {"curve": NAMES[cid], "r_f": r_f, "r_p": r_p, "products_per_permutation": products, "exact": bool(exact),
            "modmul_rate_per_s": round(rate.value, 0), "modmul_rate_field": "base field of " + NAMES[RATE_CURVE[cid]],
            "hash": rows, "merkle_2^%d_leaves" % tree_log: merkle, "merkle_tail_in_force": L.h2_poseidon_merkle_tail(),
            "tail_sweep": sweep, "product_form": product}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--curves", default="bn254,pallas,vesta")
    ap.add_argument("--max-log-n", type=int, default=22)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.reps >= 3 and 12 <= args.max_log_n <= 26
    h2.init(0)
    doc = {"tool": "tools/poseidon_bench.py",
           "timing": "HIP events around up to %d calls per window, %d windows, best / median / spread" % (args.iters, args.reps),
           "fields": [bench_field(_lib.CURVES[c], args) for c in args.curves.split(",")]}
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0 if all(f["exact"] for f in doc["fields"]) else 1


if __name__ == "__main__":
    sys.exit(main())
