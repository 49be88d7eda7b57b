"""N Poseidon k = 16 proofs through h2_generate_proof with the key kept (the call bench.py's create_proof_ms times), OS
randomness, after five warm-up calls: min / p10 / median / p90 of the wall clock per call in ms, one JSON line.
python tools/proof_loop.py [N]  -- parent-against-branch comparisons run it alternately on both builds."""
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import halo2_prover_amd as h2
from halo2_prover_amd import lib as h2lib, prover
N = int(sys.argv[1]) if len(sys.argv) > 1 else 300
k = 16
h2.init(0)
L = h2.load()
cap = 4 + 128 * (1 << k) + 256
pbuf = ctypes.create_string_buffer(cap)
ln = ctypes.c_size_t(0)
h2lib.check(L.h2_setup(k, None, None, pbuf, cap, ctypes.byref(ln)), "h2_setup")
params = pbuf.raw[:ln.value]
js = ('{"x":[1,2],"output":"0x%064x"}' % prover.PoseidonCircuit([1, 2]).output()).encode()
out = ctypes.create_string_buffer(1 << 16)
ts = []
for i in range(N + 5):
    t = time.perf_counter()
    h2lib.check(L.h2_generate_proof(params, len(params), js, 2, None, None, out, 1 << 16, ctypes.byref(ln)), "prove")
    ts.append((time.perf_counter() - t) * 1e3)
ts = sorted(ts[5:])
print(json.dumps({"n": N, "min": round(ts[0], 4), "p10": round(ts[N // 10], 4), "median": round(ts[N // 2], 4), "p90": round(ts[N * 9 // 10], 4)}))
