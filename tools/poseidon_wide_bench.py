"""The wide Poseidon family (h2_poseidon_wide_*: width 5 / arity 4 with (8, 60), width 9 / arity 8 with (8, 63)) timed
against the binary calls on the same leaves, every leg on this build in the same run, the routes alternating window by window.

Per scalar field (--curves, default Pallas and BN254; the binary calls run the field's default rounds):
  (p) permute  n states through h2_poseidon_wide_permute_device with dense and with sparse partial rounds
               (h2_selftest_set_poseidon_wide_form 1 / 2), n = 2^10, 2^16, 2^20: which form a width keeps.
  (t) tree     h2_poseidon_merkle_device at depth 20 against the 4-ary tree at depth 10 (2^20 leaves), and at depth 21
               against the 8-ary tree at depth 7 (2^21 leaves).
  (v) verify   n membership paths, n = 2^4, 2^10, 2^14, 2^17: h2_poseidon_merkle_verify_device at depth 20 on one lane and on a
               quad per hash against the wide verify at depth 10 (arity 4) and 7 (arity 8, its own 2^21-leaf tree).
  (h) hash     h2_poseidon_hash_device on 2-word messages against h2_poseidon_wide_hash_device on 4- and 8-word messages,
               n = 2^10, 2^16, 2^20: time per hash and per absorbed word.
Before anything is timed the wide paths the device cuts are verified against the wide tree's root (every status 0) and the
two forms of the permutation kernel are compared byte for byte.  After --warmup calls, --reps windows of calls between two
HIP events on the stream the calls run on: best, median, spread.  Prints one JSON document; --out FILE also writes it.
Needs the GPU, no fallback.
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import halo2_prover_amd as h2  # noqa: E402
from halo2_prover_amd import lib as _lib  # noqa: E402
from halo2_prover_amd import poseidon  # noqa: E402
from poseidon_bench import NAMES, elements, stream  # noqa: E402
from poseidon_merkle_bench import ptr, windows  # noqa: E402

WIDE = {5: (8, 60, 2), 9: (8, 63, 3)}        # width -> r_f, r_p, log2 of the arity


def bench_field(cid, args):
    import torch
    L = _lib.load()
    r_f, r_p = poseidon.DEFAULT_ROUNDS[cid]
    checks = {}

    def knob(setter, which):
        return lambda: _lib.check(setter(which), "set form")

    def nothing():
        pass

    def reps_iters(n):
        return (args.reps, max(1, min(args.iters, (1 << 12) // max(n, 1)))) if n <= (1 << 16) else (3, 1)

    # (p) the permutation kernel, dense against sparse
    permute = []
    for t, (wf, wp, _) in WIDE.items():
        states = elements(t << 20, 0x9E50 + cid + t)
        out = torch.empty_like(states)

        def run(n, t=t, wf=wf, wp=wp, states=states, out=out):
            assert L.h2_poseidon_wide_permute_device(cid, t, wf, wp, ptr(states), ptr(out), n, stream()) == 0

        results = []
        for which in (1, 2):
            knob(L.h2_selftest_set_poseidon_wide_form, which)()
            run(4096)
            results.append(out[:4096 * t].clone())
        checks["permute_width_%d_forms_agree" % t] = bool(torch.equal(results[0], results[1]))
        for log_n in (10, 16, 20):
            n = 1 << log_n
            reps, iters = reps_iters(n)
            tm = windows({"dense": (knob(L.h2_selftest_set_poseidon_wide_form, 1), lambda: run(n)),
                          "sparse": (knob(L.h2_selftest_set_poseidon_wide_form, 2), lambda: run(n))}, reps, iters, args.warmup)
            permute.append({"width": t, "log_n": log_n, **tm,
                            "sparse_over_dense": round(tm["sparse"]["best_us"] / tm["dense"]["best_us"], 3)})
        knob(L.h2_selftest_set_poseidon_wide_form, 0)()
        del states, out

    # (t), (v): binary trees of 2^20 and 2^21 leaves, the wide trees on the same leaves
    leaves = elements(1 << 21, 0x3E4C + cid)
    trees, verify = [], []
    g = torch.Generator(device="cuda")
    g.manual_seed(0x1DC5 + cid)
    nv = 1 << 17
    status = torch.empty((nv,), dtype=torch.int32, device="cuda")
    roots = torch.empty((nv, 4), dtype=torch.int64, device="cuda")
    for t, bdepth in ((5, 20), (9, 21)):
        wf, wp, lg = WIDE[t]
        a, wdepth, count = t - 1, bdepth // lg, 1 << bdepth
        bnodes = torch.empty((count - 1, 4), dtype=torch.int64, device="cuda")
        wnodes = torch.empty(((count - 1) // (a - 1), 4), dtype=torch.int64, device="cuda")

        def binary(bdepth=bdepth, bnodes=bnodes):
            assert L.h2_poseidon_merkle_device(cid, r_f, r_p, ptr(leaves), bdepth, ptr(bnodes), stream()) == 0

        def wide(t=t, wf=wf, wp=wp, wdepth=wdepth, wnodes=wnodes):
            assert L.h2_poseidon_wide_merkle_device(cid, t, wf, wp, ptr(leaves), wdepth, ptr(wnodes), stream()) == 0

        tm = windows({"binary": (nothing, binary), "wide": (nothing, wide)}, args.reps, 1, args.warmup)
        trees.append({"leaves_log2": bdepth, "binary_depth": bdepth, "arity": a, "wide_depth": wdepth, **tm,
                      "wide_over_binary": round(tm["wide"]["best_us"] / tm["binary"]["best_us"], 3)})

        idx = torch.randint(0, count, (nv,), device="cuda", generator=g).to(torch.int32)
        vals = leaves[idx.long()].contiguous()
        wpaths = torch.empty((nv, wdepth * (a - 1), 4), dtype=torch.int64, device="cuda")
        assert L.h2_poseidon_wide_merkle_paths_device(cid, t, ptr(leaves), ptr(wnodes), wdepth, ptr(idx), nv, ptr(wpaths), ptr(status),
                                                      stream()) == 0
        wroot = wnodes[-1]

        def wverify(n, t=t, wf=wf, wp=wp, wdepth=wdepth, idx=idx, vals=vals, wpaths=wpaths, wroot=wroot):
            assert L.h2_poseidon_wide_merkle_verify_device(cid, t, wf, wp, ptr(vals), ptr(idx), ptr(wpaths), wdepth, n, ptr(wroot),
                                                           ptr(roots), ptr(status), stream()) == 0

        wverify(4096)
        checks["verify_arity_%d_all_ok" % a] = not bool(status[:4096].any().item())
        routes_of = {"wide": lambda n: (nothing, lambda: wverify(n))}
        if t == 5:          # the yardstick: the binary walker at depth 20, both of its forms
            bpaths = torch.empty((nv, bdepth, 4), dtype=torch.int64, device="cuda")
            assert L.h2_poseidon_merkle_paths_device(cid, ptr(leaves), ptr(bnodes), bdepth, ptr(idx), nv, ptr(bpaths), ptr(status),
                                                     stream()) == 0
            broot = bnodes[-1]

            def bverify(n, idx=idx, vals=vals, bpaths=bpaths, broot=broot, bdepth=bdepth):
                assert L.h2_poseidon_merkle_verify_device(cid, r_f, r_p, ptr(vals), ptr(idx), ptr(bpaths), bdepth, n, ptr(broot), ptr(roots),
                                                          ptr(status), stream()) == 0

            routes_of["binary_lane"] = lambda n: (knob(L.h2_selftest_set_poseidon_walk_form, 1), lambda: bverify(n))
            routes_of["binary_quad"] = lambda n: (knob(L.h2_selftest_set_poseidon_walk_form, 2), lambda: bverify(n))
        for log_n in (4, 10, 14, 17):
            n = 1 << log_n
            reps, iters = reps_iters(n)
            tm = windows({name: make(n) for name, make in routes_of.items()}, reps, iters, args.warmup)
            verify.append({"arity": a, "wide_depth": wdepth, "log_n": log_n, **tm})
        knob(L.h2_selftest_set_poseidon_walk_form, 0)()
        del bnodes, wnodes, wpaths

    # (h) hashes of one permutation each: 2, 4 and 8 absorbed words
    hashes = []
    msgs = elements(8 << 20, 0x5A17 + cid)
    out = torch.empty((1 << 20, 4), dtype=torch.int64, device="cuda")
    for log_n in (10, 16, 20):
        n = 1 << log_n

        def h3():
            assert L.h2_poseidon_hash_device(cid, r_f, r_p, ptr(msgs), 2, 2, n, ptr(out), stream()) == 0

        def hw(t):
            wf, wp, _ = WIDE[t]
            return lambda: _lib.check(L.h2_poseidon_wide_hash_device(cid, t, wf, wp, ptr(msgs), t - 1, t - 1, n, ptr(out),
                                                                     stream()), "wide hash")

        reps, iters = reps_iters(n)
        tm = windows({"width_3": (nothing, h3), "width_5": (nothing, hw(5)), "width_9": (nothing, hw(9))}, reps, iters, args.warmup)
        hashes.append({"log_n": log_n, **tm,
                       "ns_per_word": {k: round(v["best_us"] * 1e3 / n / w, 3) for (k, v), w in zip(tm.items(), (2, 4, 8))}})
    return {"curve": NAMES[cid], "binary_rounds": [r_f, r_p], "wide_rounds": {str(t): list(v[:2]) for t, v in WIDE.items()},
            "checks": checks, "p_permute": permute, "t_tree": trees, "v_verify": verify, "h_hash": hashes}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--curves", default="pallas,bn254")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.reps >= 3
    h2.init(0)
    doc = {"tool": "tools/poseidon_wide_bench.py",
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
