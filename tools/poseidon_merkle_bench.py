"""h2_poseidon_merkle_{paths,verify,update}_device on a resident tree of 2^depth leaves (default 20), timed on both forms
of the walker -- one lane per hash and the four lanes of a quad per hash (h2_selftest_set_poseidon_walk_form 1 / 2) --
against what a host has to do without them, every leg on this build in the same run, the routes alternating window by window.

Per scalar field (--curves, default Pallas (8, 56) and BN254 (8, 60)):
  (a) verify   n membership paths, n = 1 .. 2^16 for the table and up to 2^--max-log-n for the form sweep: lane, quad, and
               `today`: `depth` calls of h2_poseidon_hash_device on pairs the host gathers level by level (torch.where on the
               index bit, one stack per level; the gather is part of what it has to do and is inside the window).
  (b) update   n distinct random leaves, n = 1 .. 2^18 and on to every leaf: lane, quad, the choice by size (form 0), and a full
               h2_poseidon_merkle_device rebuild of the tree.
  (c) single   one permutation: verify at depth 1 with one item, quad against lane.
Before anything is timed the paths the device cuts are verified against the tree's root (every status 0) and an update is
compared with a rebuild, byte for byte.  After --warmup calls, --reps windows of calls between two HIP events on the stream
the calls run on: best, median, spread.  Prints one JSON document; --out FILE also writes it.  Needs the GPU, no fallback.
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import halo2_prover_amd as h2  # noqa: E402
from halo2_prover_amd import lib as _lib  # noqa: E402
from halo2_prover_amd import poseidon  # noqa: E402
from poseidon_bench import NAMES, elements, stream, summary  # noqa: E402

P = ctypes.c_void_p


def ptr(t):
    return None if t is None else P(t.data_ptr())


def windows(routes, reps, iters, warmup):
    """routes: name -> (prepare, call); the routes alternate window by window, `prepare` runs outside the window"""
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
    depth = args.depth
    width = 1 << depth
    leaves = elements(width, 0x3E4C + cid)
    nodes = torch.empty((width - 1, 4), dtype=torch.int64, device="cuda")

    def rebuild(dst=nodes, src=leaves):
        assert L.h2_poseidon_merkle_device(cid, r_f, r_p, ptr(src), depth, ptr(dst), stream()) == 0

    def form(which):
        return lambda: _lib.check(L.h2_selftest_set_poseidon_walk_form(which), "set walk form")

    rebuild()
    root = nodes[-1]
    g = torch.Generator(device="cuda")
    g.manual_seed(0x1DC5 + cid)
    nmax = 1 << max(args.max_log_n, 18)
    all_idx = torch.randperm(width, device="cuda", generator=g)[:nmax].to(torch.int32)       # distinct leaves
    paths = torch.empty((1 << args.max_log_n, depth, 4), dtype=torch.int64, device="cuda")
    status = torch.empty((nmax,), dtype=torch.int32, device="cuda")
    roots = torch.empty((1 << args.max_log_n, 4), dtype=torch.int64, device="cuda")
    nv = 1 << args.max_log_n
    assert L.h2_poseidon_merkle_paths_device(cid, ptr(leaves), ptr(nodes), depth, ptr(all_idx), nv, ptr(paths), ptr(status), stream()) == 0
    leaf_values = leaves[all_idx[:nv].long()].contiguous()

    def verify(n, d=depth, pth=paths, want=root):
        assert L.h2_poseidon_merkle_verify_device(cid, r_f, r_p, ptr(leaf_values), ptr(all_idx), ptr(pth), d, n, ptr(want), ptr(roots),
                                                  ptr(status), stream()) == 0

    def today(n):
        """what a host does without the call: per level, order the pairs by the index bit and hash them"""
        cur, idx = leaf_values[:n], all_idx[:n].long()
        for l in range(depth):
            bit = ((idx >> l) & 1).bool().unsqueeze(1)
            sib = paths[:n, l]
            pairs = torch.stack([torch.where(bit, sib, cur), torch.where(bit, cur, sib)], dim=1)
            out = torch.empty((n, 4), dtype=torch.int64, device="cuda")
            assert L.h2_poseidon_hash_device(cid, r_f, r_p, ptr(pairs), 2, 2, n, ptr(out), stream()) == 0
            cur = out
        return cur

    def nothing():
        pass

    # exactness first
    checks = {}
    for which in (1, 2):
        form(which)()
        verify(min(nv, 4096))
        checks["verify_form_%d_all_ok" % which] = not bool(status[:min(nv, 4096)].any().item())
    form(0)()
    checks["today_route_reaches_the_root"] = bool((today(64) == root).all().item())

    def reps_iters(n):
        return (args.reps, max(1, min(args.iters, (1 << 12) // max(n, 1)))) if n <= (1 << 16) else (3, 1)

    table_a, sweep = [], []
    for log_n in range(0, args.max_log_n + 1):
        n = 1 << log_n
        in_table = log_n <= 16 and (log_n % 2 == 0)
        in_sweep = log_n >= 4
        if not (in_table or in_sweep):
            continue
        routes = {"lane": (form(1), lambda: verify(n)), "quad": (form(2), lambda: verify(n))}
        if in_table:
            routes["today"] = (nothing, lambda: today(n))
        reps, iters = reps_iters(n)
        t = windows(routes, reps, iters, args.warmup)
        row = {"log_n": log_n, **{k: v for k, v in t.items()}}
        if in_table:
            table_a.append(row)
        if in_sweep:
            sweep.append({"log_n": log_n, "lane_us": t["lane"]["best_us"], "quad_us": t["quad"]["best_us"],
                          "quad_over_lane": round(t["quad"]["best_us"] / t["lane"]["best_us"], 3)})
    form(0)()

    # (b) update: a copy of the tree is updated over and over with the same items (the same work every call)
    up_leaves, up_nodes = leaves.clone(), nodes.clone()
    values = elements(nmax, 0xABCD + cid)

    def update(n):
        assert L.h2_poseidon_merkle_update_device(cid, r_f, r_p, ptr(up_leaves), ptr(up_nodes), depth, ptr(all_idx), ptr(values), n,
                                                  ptr(status), stream()) == 0

    scratch_nodes = torch.empty_like(nodes)
    for which in (1, 2):
        form(which)()
        update(1000)
        rebuild(scratch_nodes, up_leaves)
        checks["update_form_%d_equals_rebuild" % which] = bool(torch.equal(scratch_nodes, up_nodes)) and not bool(status[:1000].any().item())
    form(0)()
    table_b = []
    for log_n in (0, 2, 4, 6, 8, 10, 12, 14, 16, 17, 18, 19, 20):         # beyond 2^18: where does the rebuild become cheaper?
        if log_n > min(depth, args.max_log_n):
            continue
        n = 1 << log_n
        routes = {"lane": (form(1), lambda: update(n)), "quad": (form(2), lambda: update(n)), "by_size": (form(0), lambda: update(n)),
                  "rebuild": (form(0), lambda: rebuild(scratch_nodes))}
        reps, iters = reps_iters(n)
        table_b.append({"log_n": log_n, **windows(routes, reps, min(iters, 4), args.warmup)})
    form(0)()
    cheaper = [r["log_n"] for r in table_b if r["rebuild"]["best_us"] < r["by_size"]["best_us"]]

    # (c) one permutation
    one_path, one_index = paths[:1, :1].contiguous(), torch.zeros((4,), dtype=torch.int32, device="cuda")

    def single_call():
        assert L.h2_poseidon_merkle_verify_device(cid, r_f, r_p, ptr(leaf_values), ptr(one_index), ptr(one_path), 1, 1, None, ptr(roots),
                                                  ptr(status), stream()) == 0

    single = windows({"lane": (form(1), single_call), "quad": (form(2), single_call)}, args.reps + 4, 16, args.warmup)
    checks["single_call_hashed"] = int(status[0].item()) == 0
    form(0)()
    return {"curve": NAMES[cid], "r_f": r_f, "r_p": r_p, "depth": depth, "checks": checks,
            "dependent_products": {"lane": 18 * r_f + 12 * r_p, "quad": 4 * (r_f + r_p)},
            "a_verify": table_a, "form_sweep_verify": sweep, "b_update": table_b,
            "b_rebuild_cheaper_from_log_n": min(cheaper) if cheaper else None,
            "c_single_permutation": {**single, "quad_over_lane": round(single["quad"]["best_us"] / single["lane"]["best_us"], 3)}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--curves", default="pallas,bn254")
    ap.add_argument("--depth", type=int, default=20)
    ap.add_argument("--max-log-n", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.reps >= 3 and 19 <= args.depth <= 24 and 16 <= args.max_log_n <= args.depth
    h2.init(0)
    doc = {"tool": "tools/poseidon_merkle_bench.py",
           "timing": "HIP events around up to %d calls per window, %d windows (3 of one call above 2^16 items), best / median / spread"
                     % (args.iters, args.reps),
           "fields": [bench_field(_lib.CURVES[c], args) for c in args.curves.split(",")]}
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0 if all(all(f["checks"].values()) for f in doc["fields"]) else 1


if __name__ == "__main__":
    sys.exit(main())
