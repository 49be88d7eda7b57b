"""Batch verification, the parts that need no GPU: the G1 decompression routine (csrc/h2_decompress.hpp) through its host
instantiation against Python big integers, and the entry point's behaviour without h2_init.

The routine under test is the text the gfx950 kernel runs, one lane per point; tests/test_gpu_verify_batch.py runs the
kernel on the same inputs.  Everything is compared exactly.
"""
import ctypes
import os
import random

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
Q = 21888242871839275222246405745257275088696311157297823662689037894645226208583      # BN254 base field
RECORDED = ("proof_arithmetic_k4.bin", "proof_poseidon_k6.bin", "proof_collatz_k10.bin")
IDENTITY_ENCODINGS = (bytes(31) + b"\x80", bytes(32))            # the two used in test_capi_product.py


@pytest.fixture(scope="module")
def lib():
    import halo2_prover_amd
    return halo2_prover_amd.load()


def expected(word):
    """(x, y, status) of one 32-byte word, as verifier.py's read_point decides (the status codes of include/h2hip.h)"""
    v = int.from_bytes(word, "little")
    sign, inf = (v >> 254) & 1, (v >> 255) & 1
    x = v & ((1 << 254) - 1)
    if x >= Q:
        return 0, 0, 1
    if inf or (x == 0 and sign == 0):
        return 0, 0, 2
    y2 = (x * x * x + 3) % Q
    y = pow(y2, (Q + 1) // 4, Q)
    if y * y % Q != y2:
        return 0, 0, 3
    if (y & 1) != sign:
        y = (Q - y) % Q
    return x, y, 0


def compress(x, sign, inf=0):
    return (x | (sign << 254) | (inf << 255)).to_bytes(32, "little")


def fixed_inputs():
    """the edge cases, then every 32-byte word of the three recorded proofs (their points, and their scalars read as points)"""
    words = []
    for x in (Q, Q + 1, (1 << 254) - 1):
        words += [compress(x, 0), compress(x, 1), compress(x, 0, 1)]          # not canonical, whatever the flags say
    words += list(IDENTITY_ENCODINGS)
    words += [compress(0, 1), compress(5, 1, 1), compress(Q - 1, 0), compress(Q - 1, 1), compress(1, 0), compress(1, 1)]
    for name in RECORDED:
        raw = open(os.path.join(GOLDEN, name), "rb").read()
        words += [raw[i:i + 32] for i in range(0, len(raw), 32)]
    return words


def input_mix(count, seed):
    """`count` compressed points: fixed_inputs(), then random x below q with both parity bits (about half of them are
    non-residues); a count below the fixed part takes a prefix of it"""
    words = fixed_inputs()
    rnd = random.Random(seed)
    while len(words) < count:
        x = rnd.randrange(Q)
        words += [compress(x, 0), compress(x, 1)]
    return words[:count]


def host_decompress(L, words):
    data = b"".join(words)
    cap = 65 * len(words)
    out = ctypes.create_string_buffer(cap)
    n = ctypes.c_size_t(0)
    assert L.h2_selftest_host(8, data, len(data), out, cap, ctypes.byref(n)) == 0
    assert n.value == cap
    raw = out.raw
    return [(int.from_bytes(raw[65 * i:65 * i + 32], "little"), int.from_bytes(raw[65 * i + 32:65 * i + 64], "little"),
             raw[65 * i + 64]) for i in range(len(words))]


def test_recorded_proofs_hold_points_the_routine_accepts():
    """the inputs are what they claim to be: the leading commitments of each recorded proof are points on the curve"""
    for name in RECORDED:
        raw = open(os.path.join(GOLDEN, name), "rb").read()
        for i in range(2):
            x, y, st = expected(raw[32 * i:32 * i + 32])
            assert st == 0 and (y * y - x * x * x - 3) % Q == 0


def test_host_decompression_matches_big_integers(lib):
    words = input_mix(len(fixed_inputs()) + 4000, 20240229)        # 2000 random x, both parities
    got = host_decompress(lib, words)
    want = [expected(w) for w in words]
    seen = {st: sum(1 for w in want if w[2] == st) for st in range(4)}
    assert min(seen.values()) > 0 and seen[3] > 1500 and seen[0] > 1500, seen
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, words[i].hex(), g, w)


def test_edge_cases_one_by_one(lib):
    cases = {compress(Q, 0): 1, compress(Q + 1, 1): 1, compress((1 << 254) - 1, 0): 1, compress(Q, 0, 1): 1,
             IDENTITY_ENCODINGS[0]: 2, IDENTITY_ENCODINGS[1]: 2, compress(7, 0, 1): 2}
    for word, status in cases.items():
        assert host_decompress(lib, [word]) == [(0, 0, status)], word.hex()
    # x = 0 with parity 1 is a point like any other: y^2 = 3
    x, y, st = host_decompress(lib, [compress(0, 1)])[0]
    assert (x, y, st) == expected(compress(0, 1))
    # (1, 2) is the generator; its negative has the odd y
    assert host_decompress(lib, [compress(1, 0)]) == [(1, 2, 0)]
    assert host_decompress(lib, [compress(1, 1)]) == [(1, Q - 2, 0)]
    assert lib.h2_selftest_host(8, b"x" * 33, 33, None, 0, None) == -1          # not a multiple of 32 bytes


NOT_INITIALISED = r"""
import ctypes, os, sys
sys.path.insert(0, sys.argv[1])
import halo2_prover_amd
lib = halo2_prover_amd.load()
golden = os.path.join(sys.argv[1], "tests", "golden")
params = open(os.path.join(golden, "params_k4.bin"), "rb").read()
proof = open(os.path.join(golden, "proof_arithmetic_k4.bin"), "rb").read()
proofs = (ctypes.c_char_p * 1)(proof)
lens = (ctypes.c_size_t * 1)(len(proof))
jsons = (ctypes.c_char_p * 1)(b'{"x":6,"y":9,"constant":7,"z":2923}')
ok = (ctypes.c_int * 1)(7)
all_ok = ctypes.c_int(7)
rc = lib.h2_verify_proofs(params, len(params), 1, proofs, lens, jsons, 1, None, None, ok, ctypes.byref(all_ok))
assert (rc, ok[0], all_ok.value) == (-5, 0, 0), (rc, ok[0], all_ok.value)
assert lib.h2_verify_proofs(params, len(params), 0, None, None, None, 1, None, None, None, ctypes.byref(all_ok)) == -5
assert lib.h2_points_decompress_device(0, None, 1, None, None, None) == -5
assert lib.h2_version() == 1002
print("not initialised: ok")
"""


def test_batch_verification_fails_loudly_without_init():
    """no CPU fallback: without h2_init the batch entry points return H2_ENOTINIT, as h2_verify_proof does (a process
    of its own, so that it holds whether or not another test has initialised the library)"""
    import subprocess
    import sys
    r = subprocess.run([sys.executable, "-c", NOT_INITIALISED, ROOT], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "not initialised: ok" in r.stdout, r.stdout + r.stderr


def test_python_wrappers_are_exported():
    import halo2_prover_amd
    assert callable(halo2_prover_amd.verify_proofs) and callable(halo2_prover_amd.points_decompress_device)
    assert "h2_verify_proofs" in halo2_prover_amd.SYMBOLS and "h2_points_decompress_device" in halo2_prover_amd.SYMBOLS
