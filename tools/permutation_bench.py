"""h2_permutation_product_device timed against the sequence of public calls it replaces.

Both build the permutation argument's grand products (halo2_proofs src/plonk/permutation/prover.rs `Argument::commit`) of
m instances over bn256::Fr on the same resident columns, in one process:
  new   one h2_permutation_product_device call for all sets of all instances
  old   what prover.py issued before that call existed, per instance and per set: about six pointwise calls per column
        (v + gamma, omega_col * beta delta^j, sigma_j * beta, two adds, two running products), h2_poly_inverse_device over
        the whole column, h2_poly_prefix_product_device, the scale by last_z and the 32-byte read-back of the set's tail,
        through the helper class (prover._Dev) the prover used; the two helpers it no longer has are restated here
The blinding rows and the RNG draws belong to neither.  Before anything is timed, rows [0, u] of every z column of the
two are compared byte for byte.

Shapes: the (k, n_cols, chunk_len) of the three circuits of the product surface as prover.py declares them (arithmetic
k = 4, Collatz k = 10, Poseidon k = 16) at m = 1 and m = 16, and one throughput-bound shape (2^22 ratio rows in one call).
After --warmup rounds of both, --reps (>= 5) rounds alternate a window of `iters` new calls and a window of `iters` old
sequences, each between two HIP events on the caller's stream (the old sequence waits for the device by itself, once per
set); best, median and spread (max - min over the windows) are microseconds per call.

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
from halo2_prover_amd import lib as h2lib  # noqa: E402
from halo2_prover_amd import prover  # noqa: E402
from halo2_prover_amd.domain import EvaluationDomain  # noqa: E402

P = prover.P
SHAPES = [  # name, k, permutation columns, degree (chunk_len = degree - 2)
    ("arithmetic", 4, len(prover.ArithmeticCircuit.permutation_columns), prover.ArithmeticCircuit.degree),
    ("collatz", 10, len(prover.CollatzCircuit.permutation_columns), prover.CollatzCircuit.degree),
    ("poseidon", 16, len(prover.PoseidonCircuit.permutation_columns), prover.PoseidonCircuit.degree),
    ("throughput", 22, 2, 4),
]
UNUSABLE = 6     # n - u: blinding factors + 1 of the three circuits


def random_columns(torch, count, n, seed):
    """`count` columns of n canonical values as (n, 4) int64 tensors: any limbs below p are some element's Montgomery form"""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    out = []
    for _ in range(count):
        t = torch.randint(-(1 << 63), (1 << 63) - 1, (n, 4), dtype=torch.int64, device="cuda", generator=g)
        t[:, 3] = torch.randint(0, (P >> 192) - 1, (n,), dtype=torch.int64, device="cuda", generator=g)
        out.append(t.contiguous())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--window-ms", type=float, default=200.0, help="device time a timed window aims at")
    ap.add_argument("--shapes", default=",".join(s[0] for s in SHAPES))
    ap.add_argument("--m", default="1,16")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.reps >= 5
    import torch
    torch.set_num_threads(min(16, torch.get_num_threads()))
    h2.init(0)
    L = h2lib.load()
    rows = []
    for name, k, n_cols, degree in SHAPES:
        if name not in args.shapes.split(","):
            continue
        dom = EvaluationDomain(degree, k, "bn254")
        dev = prover._Dev(dom, None)
        n, u, chunk = dom.n, dom.n - UNUSABLE, degree - 2
        sets = [list(range(s, min(s + chunk, n_cols))) for s in range(0, n_cols, chunk)]
        omega_col = dev.powers(dom.omega)
        sigma = random_columns(torch, n_cols, n, 1000 + k)
        for m in ([1] if name == "throughput" else [int(x) for x in args.m.split(",")]):
            values = [random_columns(torch, n_cols, n, 2000 + 100 * k + q) for q in range(m)]
            betas = [pow(3, 5 + q, P) for q in range(m)]
            gammas = [pow(7, 11 + q, P) for q in range(m)]

            def new():
                return h2.permutation_product(dom, values, sigma, chunk, u, betas, gammas, dom.omega, prover.DELTA)

            def inverse_(t):
                h2lib.check(L.h2_poly_inverse_device(dom.curve, ctypes.c_void_p(t.data_ptr()), t.numel() // 4, dom._stream()),
                            "h2_poly_inverse_device")
                return t

            def prefix_product(col):
                out = torch.empty_like(col)
                h2lib.check(L.h2_poly_prefix_product_device(dom.curve, ctypes.c_void_p(col.data_ptr()), col.shape[0],
                                                            ctypes.c_void_p(out.data_ptr()), dom._stream()), "h2_poly_prefix_product_device")
                return out

            def old():
                out = []
                for q in range(m):
                    beta, gamma = betas[q], gammas[q]
                    gamma_col = dev.const(gamma)
                    last_z = 1
                    for cols in sets:
                        num = den = None
                        for j in cols:
                            vg = dev.add(values[q][j], gamma_col)
                            tn = dev.add_(dev.scale(omega_col, pow(prover.DELTA, j, P) * beta % P), vg)
                            td = dev.add_(dev.scale(sigma[j], beta), vg)
                            num = tn if num is None else dev.mul_(num, tn)
                            den = td if den is None else dev.mul_(den, td)
                        pref = prefix_product(dev.mul_(num, inverse_(den)))
                        z = dev.scale(pref, last_z) if last_z != 1 else pref
                        last_z = last_z * dev.to_ints(pref[u:u + 1])[0] % P
                        out.append(z)
                return out

            for _ in range(args.warmup):
                zn, zo = new(), old()
            torch.cuda.synchronize()
            same = all(torch.equal(zn.reshape(-1, n, 4)[c, :u + 1], zo[c][:u + 1]) for c in range(m * len(sets)))
            # size the windows by one timed call of each
            e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
            e0.record()
            new()
            e1.record()
            old()
            e2.record()
            e2.synchronize()
            iters = max(1, min(200, int(args.window_ms / max(e0.elapsed_time(e1), 1e-3))))
            iters_old = max(1, min(200, int(args.window_ms / max(e1.elapsed_time(e2), 1e-3))))

            def window(fn, count):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(count):
                    fn()
                b.record()
                b.synchronize()
                return a.elapsed_time(b) * 1e3 / count

            tn, to = [], []
            for _ in range(args.reps):
                tn.append(window(new, iters))
                to.append(window(old, iters_old))

            def stats(t):
                return {"best_us": round(min(t), 1), "median_us": round(float(np.median(t)), 1), "spread_us": round(max(t) - min(t), 1)}

            rows.append({"shape": name, "k": k, "n_cols": n_cols, "chunk_len": chunk, "sets": len(sets), "u": u, "m": m,
                         "same_bytes": bool(same), "new": stats(tn), "old": stats(to), "iters": {"new": iters, "old": iters_old},
                         "old_over_new": round(float(np.median(to)) / float(np.median(tn)), 2),
                         "not_slower": bool(np.median(tn) <= np.median(to) + max(max(tn) - min(tn), max(to) - min(to)))})
            del values
        del sigma, omega_col
    doc = {"tool": "tools/permutation_bench.py", "curve": "bn254", "tile": L.h2_permutation_tile(), "reps": args.reps,
           "timing": "HIP events around windows of `iters` calls, new and old alternating, microseconds per call", "rows": rows}
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0 if all(r["same_bytes"] and r["not_slower"] for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
