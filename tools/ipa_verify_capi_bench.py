"""ipa.verify_proofs_bytes (ONE h2_ipa_verify_proofs call: the replay and the checks' scalars on the device) against
ipa.verify_proofs (the host replay), and the replay kernel alone.  Writes profiles/ipa_verify_capi_times.json (or --out FILE).

* Both routes on the same N items for N = 1, 16, 256 at k = 8 and k = 16 on Pallas: wall-clock milliseconds, best of five
  after two warm-ups.  ONE proof per k is repeated under N transcripts, each behind its own prefix (nothing is cached
  between items).  Making the items -- the reading transcripts for one route, the exported midstates for the other -- is
  inside the timed region of both, as a caller pays for it.
* h2_ipa_replay_device alone at those counts, HIP events, on the decompressed points of the same proofs.
Exits non-zero when the two routes disagree about any proof or do not accept it.
"""
import argparse
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
import oracle_lib as O  # noqa: E402
from halo2_prover_amd import ipa  # noqa: E402
from halo2_prover_amd import lib as h2lib  # noqa: E402

SIZES = (1, 16, 256)
KS = (8, 16)


def limbs(values):
    buf = b"".join(int(v).to_bytes(32, "little") for v in values)
    return np.frombuffer(buf, dtype=np.uint64).reshape(-1, 4).copy()


class Rng:
    def __init__(self, seed):
        self.r = random.Random(seed)

    def __call__(self, n):
        return self.r.getrandbits(8 * n).to_bytes(n, "little")


def timed(fn, repeats=5, warmups=2):
    for _ in range(warmups):
        fn()
    best, res = None, None
    for _ in range(repeats):
        t = time.perf_counter()
        res = fn()
        dt = (time.perf_counter() - t) * 1e3
        best = dt if best is None or dt < best else best
    return best, res


def event_ms(enqueue, repeats=5, warmups=2):
    """best HIP-event time of enqueue(raw stream handle)"""
    import torch
    s = torch.cuda.Stream()
    best = None
    with torch.cuda.stream(s):
        for it in range(warmups + repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            enqueue(s.cuda_stream)
            e1.record(s)
            s.synchronize()
            ms = e0.elapsed_time(e1)
            if it >= warmups and (best is None or ms < best):
                best = ms
    return round(best, 4)


def one_proof(k, prefix):
    cid, n = 1, 1 << k
    pts = O.synth_bases(cid, 0x49564300 + 16 * k + cid, n + 2).reshape(n + 2, 8)
    params = ipa.ParamsIPA("pallas", k, pts[:n], pts[n + 1], pts[n])
    p = params.p
    rnd = random.Random(0xBE7C4 + k)
    R = (1 << 256) % p
    poly = [rnd.randrange(p) for _ in range(n)]
    blind, x3 = rnd.randrange(p), rnd.randrange(1, p)
    poly_m = limbs([c * R % p for c in poly])
    v = params.domain.eval_polynomial(params.column(poly_m).reshape(1, n, 4), x3)[0]
    tr = h2.Blake2bTranscript("pallas")
    tr.state.update(prefix)
    proof = ipa.create_proof(params, tr, poly_m, blind, x3, Rng(k))
    return params, dict(P=params.commit(poly_m, blind), x3=x3, v=v, proof=proof, prefix=prefix)


def replay_ms(L, k, n, e):
    """h2_ipa_replay_device alone on n copies of the proof"""
    import torch
    per = 2 * k + 1
    mid = h2.Blake2bMidstate("pallas")
    mid.update(e["prefix"])
    d_wire = torch.frombuffer(bytearray(e["proof"][:32 * per] * n), dtype=torch.uint8).cuda()
    d_points = torch.empty(64 * per * n, dtype=torch.uint8, device="cuda")
    d_pst = torch.empty(per * n, dtype=torch.uint8, device="cuda")
    h2lib.check(L.h2_pasta_points_decompress_device(1, d_wire.data_ptr(), per * n, d_points.data_ptr(), d_pst.data_ptr(), None), "decompress")
    d_states = torch.frombuffer(bytearray(mid.export() * n), dtype=torch.uint8).cuda()
    d_scalars = torch.frombuffer(bytearray(e["proof"][32 * per:] * n), dtype=torch.uint8).cuda()
    d_out = torch.empty(32 * (k + 4) * n, dtype=torch.uint8, device="cuda")
    d_st = torch.empty(n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ms = event_ms(lambda s: h2lib.check(L.h2_ipa_replay_device(1, k, n, d_states.data_ptr(), d_points.data_ptr(), d_pst.data_ptr(),
                                                               d_scalars.data_ptr(), d_out.data_ptr(), d_st.data_ptr(), None, s), "replay"))
    assert int(d_st.cpu().sum()) == 0, "the bench's proofs must all replay"
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ipa_verify_capi_times.json"))
    ap.add_argument("--sizes", default=",".join(str(s) for s in SIZES))
    ap.add_argument("--ks", default=",".join(str(s) for s in KS))
    args = ap.parse_args()
    sizes, ks = [int(s) for s in args.sizes.split(",")], [int(s) for s in args.ks.split(",")]
    h2.init(0)
    L = h2.load()
    import torch
    result = {"device": torch.cuda.get_device_name(0), "h2_version": L.h2_version(),
              "note": "one proof per k repeated under N transcripts behind a 100-byte prefix; host = ipa.verify_proofs (the host "
                      "replay, unchanged by h2_ipa_verify_proofs), capi = ipa.verify_proofs_bytes; wall-clock ms, best of five after "
                      "two warm-ups, building the items included; replay kernel times from HIP events",
              "verify": [], "replay_kernel_ms": []}
    failures = []
    prefix = bytes(random.Random(0x50524658).getrandbits(8) for _ in range(100))
    for k in ks:
        params, e = one_proof(k, prefix)
        rows = []
        for n in sizes:
            def host():
                stats, items, t0 = {}, [], time.perf_counter()
                for _ in range(n):
                    tr = h2.Blake2bTranscript("pallas", e["proof"])
                    tr.state.update(prefix)
                    items.append((tr, e["P"], e["x3"], e["v"]))
                items_ms = (time.perf_counter() - t0) * 1e3
                got = ipa.verify_proofs(params, items, stats=stats)
                return got, dict(stats, items_ms=items_ms)

            def capi():
                stats, items, t0 = {}, [], time.perf_counter()
                for _ in range(n):
                    mid = h2.Blake2bMidstate("pallas")
                    mid.update(prefix)
                    items.append((mid.export(), e["proof"], e["P"], e["x3"], e["v"]))
                items_ms = (time.perf_counter() - t0) * 1e3
                got = ipa.verify_proofs_bytes(params, items, stats=stats)
                return got, dict(stats, items_ms=items_ms)
            host_ms, (want, host_stats) = timed(host)
            capi_ms, (got, stats) = timed(capi)
            row = {"k": k, "n": n, "host_ms": round(host_ms, 3), "capi_ms": round(capi_ms, 3), "capi_over_host": round(capi_ms / host_ms, 4),
                   "per_proof_host_ms": round(host_ms / n, 4), "per_proof_capi_ms": round(capi_ms / n, 4), "checks": stats["checks"],
                   "host_checks": host_stats["checks"], "host_items_ms": round(host_stats["items_ms"], 3),
                   "capi_items_ms": round(stats["items_ms"], 3)}
            rows.append(row)
            print(json.dumps(row), flush=True)
            if got != want or got != [True] * n:
                failures.append("k=%d n=%d: the two routes differ" % (k, n))
            krow = {"k": k, "n": n, "ms": replay_ms(L, k, n, e)}
            krow["us_per_proof"] = round(1e3 * krow["ms"] / n, 3)
            result["replay_kernel_ms"].append(krow)
            print(json.dumps(krow), flush=True)
        result["verify"].append({"k": k, "proof_bytes": len(e["proof"]), "rows": rows})
    result["failures"] = failures
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote %s" % args.out)
    for msg in failures:
        print("FAIL: " + msg, file=sys.stderr)
    return 1 if failures else 0


if __name__ == "__main__":
    sys.exit(main())
