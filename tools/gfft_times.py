"""Times of the group FFT (h2_fft_group_device) and of h2_g_to_lagrange_device, for DESIGN.md section 7.8 and
GFFT_QUAD_MAX_LOG_N (csrc/h2_tune.hpp).  Results: profiles/gfft_times.txt.

One run measures ONE build of libh2hip.so (--lib: another build, e.g. the parent commit's; the library is loaded with
plain ctypes so that a build without the newer entry points loads too): sizes 2^10, 2^14, 2^16, 2^18 (--logs) on BN254
and Pallas; per size h2_fft_group_device with the stage kernel's form chosen by size and, where the build has
h2_selftest_set_gfft_lanes, forced to one and to four lanes per butterfly, and h2_g_to_lagrange_device where the build
has it.

Method: the points are [s^i]G made on the device (h2_srs_generate), omega^-1 of the size's domain; per variant two
warm-up calls, then --reps (7, at least 5) timed calls with HIP events on the library's stream around the enqueued work
and the final synchronise, the variants of a size ALTERNATED; best, median and spread (max - min) in milliseconds.
Every call transforms the same input again (copied back before it, outside the timed window).  The forced forms and
the by-size choice must give the same points (compared after the warm-up, as bytes of the normalised g_to_lagrange
output where the build has it); the run exits non-zero when they differ.
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = {   # curve id -> (scalar modulus, multiplicative generator, two-adicity, base modulus)
    0: (0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001, 7, 28,
        0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47),
    1: (0x40000000000000000000000000000000224698FC0994A8DD8C46EB2100000001, 5, 32,
        0x40000000000000000000000000000000224698FC094CF91B992D30ED00000001),
}
NAMES = {0: "bn254", 1: "pallas"}


def limbs(v):
    return np.array([(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=os.path.join(ROOT, "halo2_prover_amd", "libh2hip.so"))
    ap.add_argument("--label", default="branch")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--logs", default="10,14,16,18")
    ap.add_argument("--out", help="append the rows as JSON lines")
    args = ap.parse_args()
    assert args.reps >= 5
    import torch   # first: one HIP runtime per process, PyTorch's
    L = ctypes.CDLL(os.path.abspath(args.lib))
    P, I, U = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32
    L.h2_init.argtypes, L.h2_srs_generate.argtypes = [I], [I, P, ctypes.c_size_t, P, P]
    L.h2_fft_group_device.argtypes = [I, P, P, U, P]
    has_lanes, has_lagrange = hasattr(L, "h2_selftest_set_gfft_lanes"), hasattr(L, "h2_g_to_lagrange_device")
    if has_lagrange:
        L.h2_g_to_lagrange_device.argtypes = [I, P, U, P, P, P, P]
    assert L.h2_init(0) == 0

    def check(st, what):
        if st != 0:
            raise RuntimeError("%s failed: %d" % (what, st))

    def timed(fns, restore):
        times = {k: [] for k in fns}
        for rep in range(2 + args.reps):
            for name, fn in fns.items():
                restore()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                if rep >= 2:
                    times[name].append(e0.elapsed_time(e1))
        return {k: {"best_ms": min(t), "median_ms": float(np.median(t)), "spread_ms": max(t) - min(t)} for k, t in times.items()}

    rows, ok = [], True
    for curve in (0, 1):
        r, gen, S, q = FIELDS[curve]
        R = (1 << 256)
        one_q = torch.from_numpy(limbs(R % q).view(np.int64)).cuda()
        for lg in [int(x) for x in args.logs.split(",")]:
            n = 1 << lg
            omega = pow(pow(gen, (r - 1) >> S, r), 1 << (S - lg), r)
            w_inv, n_inv = limbs(pow(omega, -1, r) * R % r), limbs(pow(n, -1, r) * R % r)
            aff = torch.empty((n, 8), dtype=torch.int64, device="cuda")
            s = limbs(0x1234567 * R % r)
            check(L.h2_srs_generate(curve, s.ctypes.data, n, aff.data_ptr(), None), "h2_srs_generate")
            jac0 = torch.cat([aff, one_q.expand(n, 4)], dim=1).contiguous()
            jac, lag = jac0.clone(), torch.empty_like(aff)
            torch.cuda.synchronize()

            def restore():
                jac.copy_(jac0)

            def fft(lanes):
                def run():
                    if has_lanes:
                        L.h2_selftest_set_gfft_lanes(lanes)
                    check(L.h2_fft_group_device(curve, jac.data_ptr(), w_inv.ctypes.data, lg, None), "h2_fft_group_device")
                return run

            def lagrange(lanes):
                def run():
                    L.h2_selftest_set_gfft_lanes(lanes)
                    check(L.h2_g_to_lagrange_device(curve, aff.data_ptr(), lg, w_inv.ctypes.data, n_inv.ctypes.data, lag.data_ptr(), None),
                          "h2_g_to_lagrange_device")
                return run

            fns = {"fft_by_size": fft(0)}
            if has_lanes:
                fns.update({"fft_1_lane": fft(1), "fft_4_lanes": fft(4)})
            if has_lagrange:
                fns["g_to_lagrange_by_size"] = lagrange(0)
            row = {"label": args.label, "curve": NAMES[curve], "log_n": lg, "reps": args.reps}
            try:
                if has_lagrange and has_lanes:
                    outs = []
                    for lanes in (1, 4):
                        lagrange(lanes)()
                        torch.cuda.synchronize()
                        outs.append(lag.cpu().numpy().copy())
                    row["forms_identical"] = bool(np.array_equal(outs[0], outs[1]))
                    ok &= row["forms_identical"]
                row.update(timed(fns, restore))
            finally:
                if has_lanes:
                    L.h2_selftest_set_gfft_lanes(0)
            rows.append(row)
            print(json.dumps(row), flush=True)
            del aff, jac0, jac, lag
    print("| build | curve | log n | " + " | ".join("%s median (best, spread) ms" % k for k in fns) + " |")
    print("|---|---|---|" + "---|" * len(fns))
    for row in rows:
        print("| %s | %s | %d | " % (row["label"], row["curve"], row["log_n"]) +
              " | ".join("%.3f (%.3f, %.3f)" % (row[k]["median_ms"], row[k]["best_ms"], row[k]["spread_ms"]) for k in fns) + " |")
    if args.out:
        with open(args.out, "a") as f:
            for row in rows:
                f.write(json.dumps(row) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
