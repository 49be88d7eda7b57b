"""h2_generate_proofs on the GPU, through ctypes as a Rust or JS host would call it.

The judge of every batch is the CPU oracle (oracle/halo2_ref.py create_proof, itself pinned to the reference's recorded
proofs by test_proof_pins.py): tests/golden/prove_batch_pins.json, written by tests/golden/make_prove_batch_pins.py
without the GPU library, holds the inputs and the sha256 of the oracle's proof of each under its RNG stream, and proof i
of a batch must hash to pin i.  h2_generate_proof is the same prover with a batch of one, so the second comparison --
proof i of a batch is, byte for byte, what the one-witness call returns for input i -- shows that a proof does not
depend on its neighbours or its group.  Exact comparison throughout.  The commit-phase counter tells a lockstep batch
from N one-witness calls, which would pass every byte comparison.
"""
import ctypes
import hashlib
import json
import os
import subprocess
import sys

import pytest

import pyref as R
from test_capi_product import (ARITH_INPUT, COLLATZ_INPUT, GOLDEN, POSEIDON_INPUT, PROOF_SHA256, ROOT, Stream, c_prove, c_setup,
                               c_verify, golden)
from test_gpu_verify_batch import c_verify_batch, simulate

pytestmark = pytest.mark.gpu
SIZES = [1, 2, 3, 9, 17]          # 9 passes SCAN_MAX_JOBS = 8, 17 passes MSM_MAX_MULTI = 16


@pytest.fixture(scope="module")
def lib():
    import halo2_prover_amd
    return halo2_prover_amd.load()


def start_of(i):
    return 8 + 1000 * i


def streams_rng(count, first=8):
    """one RNG_FILL callback for a batch: ctx = i + 1 draws from proof i's own recorded stream (item 0 from `first`)"""
    from halo2_prover_amd import lib as h2lib
    streams = [R.SurveyStream(start=first if i == 0 else start_of(i)) for i in range(count)]

    def fill(ctx, out, n):
        data = streams[ctx - 1].fill(n)
        for i in range(n):
            out[i] = data[i]
    return h2lib.RNG_FILL(fill), (ctypes.c_void_p * count)(*range(1, count + 1))


def c_prove_batch(L, params, jsons, idx, rng=None, ctxs=None, cap=None, fill=0xAB):
    """-> (status, proofs or None, proof_lens, out_len, the untouched-buffer flag)"""
    n = len(jsons)
    js = (ctypes.c_char_p * n)(*[j.encode() for j in jsons])
    cap = (n << 13) if cap is None else cap
    out = ctypes.create_string_buffer(bytes([fill]) * max(cap, 1), max(cap, 1))
    lens = (ctypes.c_size_t * max(n, 1))()
    total = ctypes.c_size_t(12345)
    rc = L.h2_generate_proofs(params, len(params), n, js, idx, rng, ctxs, out, cap, lens, ctypes.byref(total))
    raw = out.raw
    if rc != 0:
        return rc, None, list(lens)[:n], total.value, raw == bytes([fill]) * max(cap, 1)
    proofs, at = [], 0
    for ln in list(lens)[:n]:
        proofs.append(raw[at:at + ln])
        at += ln
    return rc, proofs, list(lens)[:n], total.value, False


def sha(proofs):
    return [hashlib.sha256(p).hexdigest() for p in proofs]


def prove_both_ways(L, params, jsons, idx, first=8):
    """the batch under per-proof streams, and the one-witness call on every item under the same streams"""
    cb, ctxs = streams_rng(len(jsons), first)
    rc, proofs, lens, total, _ = c_prove_batch(L, params, jsons, idx, cb, ctxs)
    assert rc == 0, (rc, L.h2_last_device_error())
    assert lens == [len(p) for p in proofs] and total == sum(lens)
    singles = [c_prove(L, params, js, idx, Stream(first if i == 0 else start_of(i))) for i, js in enumerate(jsons)]
    return proofs, singles


@pytest.fixture(scope="module")
def inputs(h2, lib):
    """per circuit: (params, circuit index, 17 inputs -- the recorded one first --, the oracle's proof hashes), from
    tests/golden/prove_batch_pins.json; "poseidon_k11": the hashes of the first three Poseidon inputs at k = 11.
    Collatz items 0 and 7 are both the orbit of 9 (the recorded input, and again among the orbits of 3, 4, ...): one
    witness under two RNG streams, so 17 different proofs all the same."""
    pins = json.load(open(os.path.join(GOLDEN, "prove_batch_pins.json")))
    first = {"arithmetic": ARITH_INPUT, "poseidon": POSEIDON_INPUT, "collatz": COLLATZ_INPUT}
    for name, js in first.items():
        assert pins[name]["inputs"][0] == js and len(pins[name]["inputs"]) == 17 == len(set(pins[name]["proof_sha256"]))
    for js in pins["poseidon"]["inputs"]:                             # the stored outputs are what the library computes
        item = json.loads(js)
        assert simulate(lib, '{"x":[%d,%d]}' % tuple(item["x"]), 2) == item["output"]
    p10 = c_setup(lib, 10, Stream(0))                                 # the recorded Collatz proof was made under this SRS
    out = {name: (params, idx, pins[name]["inputs"], pins[name]["proof_sha256"])
           for name, params, idx in (("arithmetic", golden("params_k4.bin"), 1), ("poseidon", golden("params_k6.bin"), 2),
                                     ("collatz", p10, 0))}
    out["poseidon_k11"] = pins["poseidon_k11"]["proof_sha256"]
    return out


RECORDED = {"arithmetic": "proof_arithmetic_k4.bin", "poseidon": "proof_poseidon_k6.bin", "collatz": "proof_collatz_k10.bin"}


@pytest.mark.parametrize("name", ["arithmetic", "poseidon", "collatz"])
@pytest.mark.parametrize("n", SIZES)
def test_batch_bytes_equal_the_single_prover(h2, lib, inputs, name, n):
    params, idx, items, pins = inputs[name]
    proofs, singles = prove_both_ways(lib, params, items[:n], idx)
    for i in range(n):
        assert hashlib.sha256(proofs[i]).hexdigest() == pins[i], (name, n, i)        # the oracle's proof of item i
        assert proofs[i] == singles[i], (name, n, i)
    assert proofs[0] == golden(RECORDED[name])                       # item 0 draws from start 8: the reference's own bytes


def test_one_larger_size(h2, lib, inputs):
    """Poseidon at k = 11, N = 3: multi-tile scans, an NTT longer than one tile"""
    rng = Stream(0)
    params = c_setup(lib, 11, rng)
    first = rng.s.counter                                             # the stream continues behind the setup
    proofs, singles = prove_both_ways(lib, params, inputs["poseidon"][2][:3], 2, first)
    assert sha(proofs) == inputs["poseidon_k11"]
    assert proofs == singles
    assert hashlib.sha256(proofs[0]).hexdigest() == PROOF_SHA256[("poseidon", 11)]


def test_groups(h2, lib, inputs):
    params, idx, items, pins = inputs["arithmetic"]
    lib.h2_selftest_set_prove_group(4)
    try:
        proofs, singles = prove_both_ways(lib, params, items[:9], idx)
    finally:
        lib.h2_selftest_set_prove_group(0)
    assert sha(proofs) == pins[:9]
    assert proofs == singles


def test_split_launch_respects_the_msm_column_limit(h2, lib, inputs):
    """Columns that bring their own bases cannot be cut into groups, so the products / random-polynomial split launch
    must fit one MSM launch sequence.  From k = 18 a sequence holds 8 columns; here the entries cap holds it to 4, so a
    Poseidon batch of 2 or 3 (6 or 9 such columns) has to take one launch per base, while the single proof (3) splits."""
    params, idx, items, pins = inputs["poseidon"]
    geom = (ctypes.c_uint64 * 8)()
    assert lib.h2_selftest_msm_check(0, 64, 64, 1, 64, 0, geom) == 0
    windows = geom[1]
    lib.h2_selftest_set_msm_max_entries(4 * windows * 64)
    try:
        for n in (2, 3):
            proofs, singles = prove_both_ways(lib, params, items[:n], idx)
            assert sha(proofs) == pins[:n], n
            assert proofs == singles, n
        assert proofs[0] == golden("proof_poseidon_k6.bin")
    finally:
        lib.h2_selftest_set_msm_max_entries(0)


@pytest.mark.parametrize("name", ["poseidon", "collatz"])
def test_lockstep_not_a_loop(h2, lib, inputs, name):
    params, idx, items, _ = inputs[name]
    c_prove(lib, params, items[0], idx, None)                         # the key is built and cached
    before = lib.h2_selftest_commit_launches()
    c_prove(lib, params, items[0], idx, None)
    d1 = lib.h2_selftest_commit_launches() - before
    assert d1 >= 4
    before = lib.h2_selftest_commit_launches()
    assert c_prove_batch(lib, params, items[:8], idx)[0] == 0
    d8 = lib.h2_selftest_commit_launches() - before
    assert d8 <= d1 + 1, (d1, d8)                                     # + 1: the products / random-polynomial split
    lib.h2_selftest_set_prove_group(4)
    try:
        before = lib.h2_selftest_commit_launches()
        assert c_prove_batch(lib, params, items[:8], idx)[0] == 0
        d8 = lib.h2_selftest_commit_launches() - before
    finally:
        lib.h2_selftest_set_prove_group(0)
    assert d8 <= 2 * (d1 + 1), (d1, d8)


def test_a_bad_witness_among_good_ones(h2, lib, inputs):
    params, idx, items, pins = inputs["arithmetic"]
    jsons = list(items[:5])
    x, y, c, z = [int(v.split(":")[1]) for v in jsons[2].strip("{}").split(",")]
    jsons[2] = '{"x":%d,"y":%d,"constant":%d,"z":%d}' % (x, y, c, z + 1)          # well-formed, false
    proofs, singles = prove_both_ways(lib, params, jsons, idx)
    assert proofs == singles
    assert [h == w for h, w in zip(sha(proofs), pins)] == [True, True, False, True, True]     # the good ones are the oracle's
    assert c_verify_batch(lib, params, list(zip(proofs, jsons)), idx) == (0, [1, 1, 0, 1, 1], 0)


@pytest.mark.parametrize("name", ["arithmetic", "poseidon", "collatz"])
def test_os_randomness(h2, lib, inputs, name):
    params, idx, items, _ = inputs[name]
    rc, proofs, lens, total, _ = c_prove_batch(lib, params, items[:16], idx)
    assert rc == 0 and total == sum(lens)
    assert len(set(lens)) == 1 and len(set(proofs)) == 16
    assert c_verify_batch(lib, params, list(zip(proofs, items[:16])), idx) == (0, [1] * 16, 1)


def test_statuses(h2, lib, inputs):
    params, idx, items, _ = inputs["arithmetic"]
    total = ctypes.c_size_t(77)
    assert lib.h2_generate_proofs(params, len(params), 0, None, idx, None, None, None, 0, None, ctypes.byref(total)) == 0
    assert total.value == 0
    rc, proofs, _, _, untouched = c_prove_batch(lib, params, [items[0], "{", items[2]], idx)
    assert (rc, proofs, untouched) == (-6, None, True)                # H2_EPROOF, nothing written
    rc, good, lens, need, _ = c_prove_batch(lib, params, items[:3], idx)
    assert rc == 0 and need == sum(lens)
    rc, proofs, _, asked, untouched = c_prove_batch(lib, params, items[:3], idx, cap=need - 1)
    assert (rc, proofs, asked, untouched) == (-1, None, need, True)   # H2_EINVAL, *out_len = the size needed
    js = (ctypes.c_char_p * 2)(*[j.encode() for j in items[:2]])
    out = ctypes.create_string_buffer(1 << 14)
    lens2 = (ctypes.c_size_t * 2)()
    args = (params, len(params), 2)
    assert lib.h2_generate_proofs(*args, None, idx, None, None, out, 1 << 14, lens2, ctypes.byref(total)) == -1
    assert lib.h2_generate_proofs(*args, js, idx, None, None, out, 1 << 14, lens2, None) == -1
    assert lib.h2_generate_proofs(*args, js, idx, None, None, out, 1 << 14, None, ctypes.byref(total)) == -1
    # circuit 7 is Poseidon, as for h2_generate_proof
    p6, _, pos, _ = inputs["poseidon"]
    cb, ctxs = streams_rng(1)
    rc, proofs, _, _, _ = c_prove_batch(lib, p6, pos[:1], 7, cb, ctxs)
    assert rc == 0 and proofs[0] == golden("proof_poseidon_k6.bin")
    assert c_prove_batch(lib, p6, [ARITH_INPUT], 7)[0] == c_prove_status(lib, p6, ARITH_INPUT, 7)


def c_prove_status(L, params, js, idx):
    n = ctypes.c_size_t(0)
    out = ctypes.create_string_buffer(1 << 16)
    return L.h2_generate_proof(params, len(params), js.encode(), idx, None, None, out, 1 << 16, ctypes.byref(n))


_TWO_CONTEXTS = r'''
import ctypes, json, os, sys
ROOT = %r
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import halo2_prover_amd as h2
from halo2_prover_amd import api
import test_capi_product as T
import test_gpu_prove_batch as B
api.init_devices([0, 0])                      # two contexts on the one GPU
L = h2.load()
assert L.h2_device_count() == 2
L.h2_selftest_set_shard_min_rows(16)          # spread the k = 6 commitments (64 rows) over the contexts
params = T.golden("params_k6.bin")
jsons = json.load(open(os.path.join(T.GOLDEN, "prove_batch_pins.json")))["poseidon"]["inputs"][:3]
before = L.h2_selftest_sharded_commits()
cb, ctxs = B.streams_rng(3)
rc, proofs, lens, total, _ = B.c_prove_batch(L, params, jsons, 2, cb, ctxs)
assert rc == 0, (rc, L.h2_last_device_error())
assert L.h2_selftest_sharded_commits() > before, "the commit phases were not spread over the two contexts"
assert proofs[0] == T.golden("proof_poseidon_k6.bin")
print("two contexts ok " + " ".join(p.hex() for p in proofs))
'''


def test_two_contexts(h2, lib, inputs):
    """the batch's commit phases spread over two contexts by point range: the bytes of the one-context one-witness calls"""
    r = subprocess.run([sys.executable, "-c", _TWO_CONTEXTS % ROOT], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "two contexts ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    got = [bytes.fromhex(h) for h in r.stdout.split("two contexts ok ")[1].split()]
    params, idx, items, pins = inputs["poseidon"]
    singles = [c_prove(lib, params, js, idx, Stream(start_of(i))) for i, js in enumerate(items[:3])]
    assert sha(got) == pins[:3]
    assert got == singles


def test_python_wrapper(h2, lib, inputs):
    params, idx, items, pins = inputs["poseidon"]
    cb, ctxs = streams_rng(3)
    rc, proofs, _, _, _ = c_prove_batch(lib, params, items[:3], idx, cb, ctxs)
    assert rc == 0 and sha(proofs) == pins[:3]
    rngs = [R.SurveyStream(start=start_of(i)).fill for i in range(3)]
    assert h2.generate_proofs(params, items[:3], idx, rngs) == proofs
    assert h2.generate_proofs(params, [], idx) == []
    fresh = h2.generate_proofs(params, items[:2], idx)
    assert [c_verify(lib, params, p, js, idx) for p, js in zip(fresh, items[:2])] == [(0, 1), (0, 1)]
