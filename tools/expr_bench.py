"""h2_expr_eval_device timed against the node-by-node evaluation it replaces.

Two programs, each on 2^16 and 2^19 rows and m in {1, 4} instances:
  poseidon_mix   a random DAG over bn256::Fr with the node mix of the Poseidon circuit's own quotient program: as many
                 arithmetic nodes, the same share of products and of column, constant and variable operands (the counters
                 of that program come from h2_selftest_host what = 6; the DAG itself is not exported)
  random_pallas  a random DAG of the same size over the Pallas scalar field
The columns are resident in HBM in the API form.  After --warmup calls a window of --iters calls sits between two HIP
events on the caller's stream, and --reps (>= 5) windows give the best, the median and the spread in microseconds per
call.

The yardstick is what a host does without the call: the same DAG node by node on scratch columns, one
h2_poly_pointwise_device (or, for a product with a constant, h2_poly_scale_device) per arithmetic node after a device copy
of its first operand (the calls work in place), scratch columns reused once their value is dead.  What that host would
also pay is NOT charged to it: the rotated copies of the columns and the constant columns are built before the clock
starts, and all m instances share every launch.  So the yardstick flatters the host.  Before anything is timed both results
are compared, limb for limb.

Prints one JSON document; --out FILE also writes it.  A measurement path: it needs the GPU and has no fallback.
"""
import argparse
import ctypes
import json
import os
import random
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import halo2_prover_amd as h2  # noqa: E402
from halo2_prover_amd import lib as h2lib  # noqa: E402
from halo2_prover_amd.domain import EvaluationDomain, _FIELDS, _limbs  # noqa: E402
from halo2_prover_amd.expr import ADD, COL, CONST, MUL, SUB, VAR  # noqa: E402

POSEIDON = 2
N_COLS, N_VARS, N_CONSTS = 12, 4, 8
ROTS = (0, 0, 0, 1, -1)


def circuit_counters(L, circuit):
    out = ctypes.create_string_buffer(1 << 20)
    n = ctypes.c_size_t(0)
    h2lib.check(L.h2_selftest_host(6, bytes([circuit]), 1, out, 1 << 20, ctypes.byref(n)), "h2_selftest_host(6)")
    names = ("instructions", "products", "column_reads", "slots", "constants", "reductions")
    return dict(zip(names, struct.unpack("<6I", out.raw[:24])))


def mixed_dag(rng, p, target):
    """arithmetic nodes = the target's instructions less its inserted reductions, products and column operands in the
    target's proportions; the other leaf operands are constants and variables, the rest earlier results.  Every result
    is used: an operand that is an earlier result takes one that nobody has read yet while there is one, and the last
    nodes fold what is left, so the compiled program has as many instructions as the DAG has arithmetic nodes."""
    n_arith = target["instructions"] - target["reductions"]
    p_mul = (target["products"] - target["reductions"]) / n_arith
    p_col = target["column_reads"] / (2.0 * n_arith)
    consts = [rng.randrange(p) for _ in range(N_CONSTS)]
    nodes, arith, unread = [], [], []

    def operand(must_fold):
        u = rng.random()
        if unread and (must_fold or u >= p_col + 0.16):
            return unread.pop(rng.randrange(max(0, len(unread) - 4), len(unread)))
        if u < p_col or not arith:
            nodes.append((COL, rng.randrange(N_COLS), 0, rng.choice(ROTS)))
        elif u < p_col + 0.08:
            nodes.append((CONST, 0, 0, rng.randrange(N_CONSTS)))
        elif u < p_col + 0.16:
            nodes.append((VAR, 0, 0, rng.randrange(N_VARS)))
        else:
            return rng.choice(arith)
        return len(nodes) - 1

    while len(arith) < n_arith:
        need, excess = n_arith - len(arith), len(unread) - 1      # nodes still to come; unread results beyond the root
        a, b = operand(excess >= need - 1), operand(excess >= need)   # towards the end every node folds two
        nodes.append((MUL if rng.random() < p_mul else rng.choice((ADD, SUB)), a, b, 0))
        arith.append(len(nodes) - 1)
        unread.append(len(nodes) - 1)
    return nodes, consts


class Yardstick:
    """the DAG node by node with the pointwise calls, on (m, rows, 4) tensors"""

    def __init__(self, dom, nodes, consts, cols, variables, rows, step):
        import torch
        self.torch, self.dom, self.nodes = torch, dom, nodes
        self.L, self.stream = dom._L, dom._stream()
        m = len(cols)
        self.shape = (m, rows, 4)
        self.leaf = {}
        for i, (op, a, b, x) in enumerate(nodes):
            if op == COL:
                self.leaf[i] = torch.stack([torch.roll(cols[q][a], -x * step, dims=0) for q in range(m)])
            elif op in (CONST, VAR):
                vals = [consts[x]] * m if op == CONST else [variables[q][x] for q in range(m)]
                t = torch.empty(self.shape, dtype=torch.int64, device="cuda")
                for q in range(m):
                    t[q] = torch.from_numpy(dom.mont(vals[q]).view(np.int64)).cuda()
                self.leaf[i] = t
        self.scalar = {i: (consts[x], dom.mont(consts[x])) for i, (op, a, b, x) in enumerate(nodes) if op == CONST}
        self.last_use = {}
        for i, (op, a, b, x) in enumerate(nodes):
            if op in (ADD, SUB, MUL):
                self.last_use[a] = self.last_use[b] = i
        self.launches = sum(1 for nd in nodes if nd[0] in (ADD, SUB, MUL))

    def run(self):
        torch, L, cid = self.torch, self.L, self.dom.curve
        val, free = dict(self.leaf), []
        for i, (op, a, b, x) in enumerate(self.nodes):
            if op not in (ADD, SUB, MUL):
                continue
            t = free.pop() if free else torch.empty(self.shape, dtype=torch.int64, device="cuda")
            if op == MUL and (a in self.scalar or b in self.scalar):
                s, o = (a, b) if a in self.scalar else (b, a)
                t.copy_(val[o])
                h2lib.check(L.h2_poly_scale_device(cid, ctypes.c_void_p(t.data_ptr()), t.numel() // 4, 1,
                                                   self.scalar[s][1].ctypes.data, self.stream), "h2_poly_scale_device")
            else:
                t.copy_(val[a])
                h2lib.check(L.h2_poly_pointwise_device(cid, {ADD: 0, SUB: 1, MUL: 2}[op], ctypes.c_void_p(t.data_ptr()),
                                                       ctypes.c_void_p(val[b].data_ptr()), t.numel() // 4, self.stream),
                            "h2_poly_pointwise_device")
            val[i] = t
            for src in {a, b}:
                if self.last_use[src] == i and src not in self.leaf:
                    free.append(val.pop(src))
        return val[len(self.nodes) - 1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--log-rows", default="16,19")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.reps >= 5 and args.iters >= 1
    import torch
    torch.set_num_threads(min(16, torch.get_num_threads()))
    h2.init(0)
    L = h2lib.load()
    target = circuit_counters(L, POSEIDON)

    def timed(fn, iters):
        times = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1) * 1e3 / iters)
        return {"best_us": round(min(times), 1), "median_us": round(float(np.median(times)), 1),
                "spread_us": round(max(times) - min(times), 1)}

    rows_out = []
    for name, curve in (("poseidon_mix", "bn254"), ("random_pallas", "pallas")):
        dom = EvaluationDomain(2, 4, curve)
        p = _FIELDS[dom.curve][0]
        rng = random.Random(0xE8 + dom.curve)
        nodes, consts = mixed_dag(rng, p, target)
        prog = h2.ExprProgram(nodes, consts, N_COLS, N_VARS, curve)
        info = prog.info()
        for log_rows in [int(k) for k in args.log_rows.split(",")]:
            rows, step = 1 << log_rows, 4
            for m in (1, 4):
                nrng = np.random.default_rng(100 * log_rows + m)

                def column():
                    t = nrng.integers(0, 1 << 64, size=(rows, 4), dtype=np.uint64)
                    t[:, 3] = nrng.integers(0, p >> 192, size=rows, dtype=np.uint64)       # canonical: below p
                    return torch.from_numpy(t.view(np.int64)).cuda()
                cols = [[column() for _ in range(N_COLS)] for _ in range(m)]
                variables = [[rng.randrange(p) for _ in range(N_VARS)] for _ in range(m)]
                out = torch.empty((m, rows, 4), dtype=torch.int64, device="cuda")
                yard = Yardstick(dom, nodes, consts, cols, variables, rows, step)

                def fused():
                    prog.eval(dom, cols, variables, log_rows, step, out=out, out_stride=rows)

                for _ in range(args.warmup):
                    fused()
                    ref = yard.run()
                torch.cuda.synchronize()
                exact = bool(torch.equal(out, ref))
                del ref
                iters = max(1, args.iters // (4 if log_rows >= 19 else 1))
                t_fused, t_yard = timed(fused, iters), timed(yard.run, max(1, iters // 2))
                rows_out.append({"program": name, "curve": curve, "log_rows": log_rows, "m": m, "exact": exact,
                                 "h2_expr_eval_device": t_fused, "node_by_node": t_yard, "node_by_node_launches": yard.launches,
                                 "iters": iters, "speedup": round(t_yard["best_us"] / t_fused["best_us"], 1)})
                del cols, yard, out
        rows_out.append({"program": name, "curve": curve, "info": info})
        prog.release()
    doc = {"tool": "tools/expr_bench.py", "poseidon_program": target, "reps": args.reps,
           "timing": "HIP events around `iters` calls, per call", "rows": rows_out}
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0 if all(r.get("exact", True) for r in rows_out) else 1


if __name__ == "__main__":
    sys.exit(main())
