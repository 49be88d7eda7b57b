"""h2_lookup_permute_device and h2_lookup_product_device timed against the host round trip they replace.

Per shape -- m in {1, 4} lookups of u in {2^12 - 6, 2^16 - 6, 2^20 - 6} usable rows over bn256::Fr, two kinds of values:
  range8      an 8-bit range table (0..255, zero padding) with uniformly drawn inputs
  random254   random 254-bit table values, about half of the input rows repeats of the other half
the columns are made resident in HBM in the API form (Montgomery limbs).  After --warmup calls a window of --iters calls
sits between two HIP events on the caller's stream, and --reps (>= 5) windows give the best, the median and the spread in
microseconds per call.  `passes` is the number of radix passes that ran for the input and the table column of lookup 0:
the byte positions on which the canonical keys of the column do not all agree, the rule the plan kernel applies on the
device (csrc/h2_lookup.hpp).

The yardstick is what a caller has to do without the calls: copy both columns of every lookup to the host, sort and
assign there, copy A' and S' back.  The host step is numpy on the canonical integers (one lexsort of the 4 x u64 limbs of
both columns into dense ranks, then sorts, searchsorted and masks on the ranks).  The conversions from and to Montgomery
form that a real host also pays are NOT charged to it, so the yardstick flatters the host.  Before anything is timed the
GPU result is compared with that host result, limb for limb.

Prints one JSON document; --out FILE also writes it.  A measurement path: it needs the GPU and has no fallback.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import halo2_prover_amd as h2  # noqa: E402
from halo2_prover_amd import lib as h2lib  # noqa: E402
from halo2_prover_amd.domain import _FIELDS  # noqa: E402

CID = 0
LOG_U = (12, 16, 20)
PAD = 6          # u = 2^k - 6, col_stride = 2^k


def limbs_of(v):
    return np.frombuffer(v.to_bytes(32, "little"), dtype=np.uint64).copy()


def make_columns(kind, u, stride, m, p, rng):
    """canonical (m, stride, 4) uint64 inputs and tables, rows [u, stride) zero"""
    A = np.zeros((m, stride, 4), dtype=np.uint64)
    S = np.zeros((m, stride, 4), dtype=np.uint64)
    for j in range(m):
        if kind == "range8":
            S[j, :256, 0] = np.arange(256, dtype=np.uint64)
            A[j, :u, 0] = rng.integers(0, 256, size=u, dtype=np.uint64)
        else:
            t = rng.integers(0, 1 << 64, size=(u, 4), dtype=np.uint64)
            t[:, 3] = rng.integers(0, p >> 192, size=u, dtype=np.uint64)          # canonical: below p
            S[j, :u] = t
            half = u // 2
            perm = rng.permutation(u)
            idx = np.concatenate([perm[:half], rng.choice(perm[:half], size=u - half)])
            A[j, :u] = t[rng.permutation(idx)]
    return A, S


def passes_of(col):
    """byte positions of the 32-byte keys on which the rows of `col` (u, 4) do not all agree"""
    b = np.ascontiguousarray(col).view(np.uint8).reshape(len(col), 32)
    return int(np.count_nonzero(np.bitwise_and.reduce(b, axis=0) != np.bitwise_or.reduce(b, axis=0)))


def host_permute(A, S):
    """canonical (u, 4) columns -> (A', S', ok) by numpy on dense ranks"""
    u = len(A)
    both = np.concatenate([A, S])
    order = np.lexsort((both[:, 0], both[:, 1], both[:, 2], both[:, 3]))
    srt = both[order]
    new = np.ones(2 * u, dtype=bool)
    new[1:] = np.any(srt[1:] != srt[:-1], axis=1)
    rank_sorted = np.cumsum(new) - 1
    values = srt[new]
    rank = np.empty(2 * u, dtype=np.int64)
    rank[order] = rank_sorted
    a = np.sort(rank[:u])
    s = np.sort(rank[u:])
    first = np.ones(u, dtype=bool)
    first[1:] = a[1:] != a[:-1]
    pos = np.searchsorted(s, a[first], side="left")
    ok = bool(np.all(pos < u) and np.all(s[np.minimum(pos, u - 1)] == a[first]))
    sp = np.zeros(u, dtype=np.int64)
    sp[first] = a[first]
    if ok:
        removed = np.zeros(u, dtype=bool)
        removed[pos] = True
        sp[np.nonzero(~first)[0][::-1]] = s[~removed]
    return values[a], values[sp], ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--log-u", default=",".join(str(k) for k in LOG_U))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.reps >= 5 and args.iters >= 1
    import torch
    torch.set_num_threads(min(16, torch.get_num_threads()))
    h2.init(0)
    L = h2lib.load()
    p = _FIELDS[CID][0]
    R = (1 << 256) % p
    to_mont, from_mont = limbs_of(R * R % p), limbs_of(1)      # raw limbs c: poly_scale computes a * c / R
    beta, gamma = limbs_of(0x1234567 * R % p), limbs_of(0x7654321 * R % p)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def scale(t, c):
        h2lib.check(L.h2_poly_scale_device(CID, ctypes.c_void_p(t.data_ptr()), t.numel() // 4, 1, c.ctypes.data, stream), "h2_poly_scale_device")

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

    rows = []
    for log_u in [int(k) for k in args.log_u.split(",")]:
        stride = 1 << log_u
        u = stride - PAD
        for kind in ("range8", "random254"):
            for m in (1, 4):
                rng = np.random.default_rng(100 * log_u + m + (7 if kind == "range8" else 0))
                A, S = make_columns(kind, u, stride, m, p, rng)
                d_in, d_tab = torch.from_numpy(A.view(np.int64)).cuda(), torch.from_numpy(S.view(np.int64)).cuda()
                scale(d_in, to_mont)
                scale(d_tab, to_mont)
                pin, ptab, z = torch.zeros_like(d_in), torch.zeros_like(d_in), torch.zeros_like(d_in)
                status = torch.zeros((m,), dtype=torch.int32, device="cuda")
                P = [ctypes.c_void_p(t.data_ptr()) for t in (d_in, d_tab, pin, ptab, status, z)]

                def permute():
                    h2lib.check(L.h2_lookup_permute_device(CID, P[0], P[1], u, stride, m, P[2], P[3], P[4], stream), "h2_lookup_permute_device")

                def product():
                    h2lib.check(L.h2_lookup_product_device(CID, P[0], P[1], P[2], P[3], u, stride, m, beta.ctypes.data, gamma.ctypes.data,
                                                           P[5], stream), "h2_lookup_product_device")

                for _ in range(args.warmup):
                    permute()
                    product()
                torch.cuda.synchronize()
                # the GPU's A' and S' against the host's, on canonical limbs
                ca, cs = pin.clone(), ptab.clone()
                scale(ca, from_mont)
                scale(cs, from_mont)
                ga, gs = ca.cpu().numpy().view(np.uint64), cs.cpu().numpy().view(np.uint64)
                exact = status.tolist() == [0] * m
                for j in range(m):
                    ha, hs, ok = host_permute(A[j, :u], S[j, :u])
                    exact = exact and ok and np.array_equal(ga[j, :u], ha) and np.array_equal(gs[j, :u], hs)
                one = limbs_of(R).view(np.int64)
                z_ends_in_one = bool(np.array_equal(z[:, u].cpu().numpy(), np.tile(one, (m, 1))))
                iters = max(1, args.iters // (4 if log_u >= 20 else 1))
                t_perm, t_prod = timed(permute, iters), timed(product, iters)
                # the round trip: both columns down, numpy, two columns up (Montgomery conversions not charged)
                trips = []
                for _ in range(3):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    ha_all, hs_all = d_in.cpu().numpy().view(np.uint64), d_tab.cpu().numpy().view(np.uint64)
                    t1 = time.perf_counter()
                    outs = [host_permute(A[j, :u], S[j, :u]) for j in range(m)]
                    t2 = time.perf_counter()
                    for j in range(m):
                        pin[j, :u].copy_(torch.from_numpy(outs[j][0].view(np.int64)))
                        ptab[j, :u].copy_(torch.from_numpy(outs[j][1].view(np.int64)))
                    torch.cuda.synchronize()
                    t3 = time.perf_counter()
                    trips.append((t3 - t0, t1 - t0, t2 - t1, t3 - t2))
                    del ha_all, hs_all
                best = min(trips)
                rows.append({"kind": kind, "log_u": log_u, "u": u, "m": m, "exact": bool(exact), "z_ends_in_one": z_ends_in_one,
                             "passes": {"input": passes_of(A[0, :u]), "table": passes_of(S[0, :u])},
                             "permute": t_perm, "product": t_prod, "iters": iters,
                             "round_trip_us": {"total": round(best[0] * 1e6, 1), "to_host": round(best[1] * 1e6, 1),
                                               "numpy": round(best[2] * 1e6, 1), "to_device": round(best[3] * 1e6, 1)},
                             "speedup_permute": round(best[0] * 1e6 / t_perm["best_us"], 1)})
                del d_in, d_tab, pin, ptab, z
    doc = {"tool": "tools/lookup_bench.py", "curve": "bn254", "tile": L.h2_lookup_tile(), "reps": args.reps,
           "timing": "HIP events around `iters` calls, per call; round trip: host clock, best of 3", "rows": rows}
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0 if all(r["exact"] and r["z_ends_in_one"] for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
