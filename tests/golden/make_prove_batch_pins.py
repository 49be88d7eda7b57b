#!/usr/bin/env python3
"""Mint prove_batch_pins.json: the inputs of tests/test_gpu_prove_batch.py and, for each, the sha256 of the proof that
the CPU oracle (oracle/halo2_ref.py create_proof on OracleBackend -- pinned to the reference's recorded proofs by
tests/test_proof_pins.py) makes of it under the RNG stream the test gives it.  CPU only; nothing of the GPU library is
used, so the hashes judge the GPU prover from outside.

Per circuit (arithmetic k = 4, Poseidon k = 6, Collatz k = 10 with SHPLONK): 17 input JSON strings, the recorded input
first, and the hash of item i's proof under SurveyStream(start = 8 if i == 0 else 8 + 1000 i).  Item 0 must hash to the
recorded proof file.  "poseidon_k11": the first three Poseidon inputs under the k = 11 SRS (item 0 continues the stream
behind setup(11), which is counter 8 again); item 0 must hash to the recorded k = 11 proof.

Takes about two minutes."""
import hashlib
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import halo2_ref as H  # noqa: E402
import pyref as R  # noqa: E402
from test_oracle_pins import params_bytes_c  # noqa: E402

COUNT = 17
ARITH_INPUT = '{"x":6,"y":9,"constant":7,"z":2923}'
COLLATZ_SEQ = [9, 28, 14, 7, 22, 11, 34, 17, 52, 26, 13, 40, 20, 10, 5, 16, 8, 4, 2, 1]
PROOF_SHA256_POSEIDON_K11 = "8d2d9052b47d9c9b45f3e3c268cec30797f74990cb47367bdfa7fbe77832129c"


def golden(name):
    return open(os.path.join(HERE, name), "rb").read()


def start_of(i):
    return 8 if i == 0 else 8 + 1000 * i


def orbit(start):
    seq = [start]
    while seq[-1] != 1:
        seq.append(seq[-1] // 2 if seq[-1] % 2 == 0 else 3 * seq[-1] + 1)
    return seq


def witnesses():
    """per circuit the test's 17 witnesses: (JSON string, oracle circuit, instance columns)"""
    rnd = random.Random(64)
    out = {}
    items = [(ARITH_INPUT, H.ArithmeticCircuit(6, 9, 7), [[7, 2923]])]
    while len(items) < COUNT:
        x, y, c = rnd.randrange(1 << 12), rnd.randrange(1 << 12), rnd.randrange(1 << 30)
        z = x * x * y * y + c
        items.append(('{"x":%d,"y":%d,"constant":%d,"z":%d}' % (x, y, c, z), H.ArithmeticCircuit(x, y, c), [[c, z]]))
    out["arithmetic"] = items
    items, msgs = [], [(1, 2)]
    while len(msgs) < COUNT:
        msgs.append((rnd.randrange(1 << 64), rnd.randrange(1 << 64)))
    for msg in msgs:
        circuit = H.PoseidonCircuit(list(msg))
        items.append(('{"x":[%d,%d],"output":"0x%064x"}' % (msg[0], msg[1], circuit.output()), circuit, [[circuit.output()]]))
    out["poseidon"] = items
    items, start = [('{"x":%s}' % str(COLLATZ_SEQ).replace(" ", ""), H.CollatzCircuit(COLLATZ_SEQ), [])], 2
    while len(items) < COUNT:
        start += 1
        seq = orbit(start)
        if len(seq) <= 32:
            items.append(('{"x":%s}' % str(seq).replace(" ", ""), H.CollatzCircuit(seq), []))
    out["collatz"] = items
    return out


def proof_hashes(params, items, opening="gwc"):
    """the key does not depend on the witness: one keygen, then every item's proof under its own stream"""
    be = H.OracleBackend(params)
    pk = H.ProvingKey(items[0][1], be)
    hashes = []
    for i, (_, circuit, instances) in enumerate(items):
        pk.circuit = circuit
        proof = H.create_proof(pk, be, instances, R.SurveyStream(start=start_of(i)), opening=opening)
        hashes.append(hashlib.sha256(proof).hexdigest())
    return hashes


def main():
    W = witnesses()
    out = {}
    for name, params, opening, recorded in (("arithmetic", golden("params_k4.bin"), "gwc", "proof_arithmetic_k4.bin"),
                                            ("poseidon", golden("params_k6.bin"), "gwc", "proof_poseidon_k6.bin"),
                                            ("collatz", params_bytes_c(10), "shplonk", "proof_collatz_k10.bin")):
        hashes = proof_hashes(params, W[name], opening)
        assert hashes[0] == hashlib.sha256(golden(recorded)).hexdigest(), name
        assert len(set(hashes)) == COUNT
        out[name] = {"inputs": [js for js, _, _ in W[name]], "proof_sha256": hashes}
        print(name, "ok", file=sys.stderr)
    hashes = proof_hashes(params_bytes_c(11), W["poseidon"][:3])
    assert hashes[0] == PROOF_SHA256_POSEIDON_K11
    out["poseidon_k11"] = {"proof_sha256": hashes}
    dst = os.path.join(HERE, "prove_batch_pins.json")
    with open(dst, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", dst)


if __name__ == "__main__":
    sys.exit(main())
