"""Square roots in the base fields and decompression of the Pasta wire form, the parts that need no GPU: the generated
constants, the host instantiations of the routines the gfx950 kernels run (h2_selftest_host, what = 10 and 11) against
Python big integers and transcript.decompress, and the entry points' behaviour without h2_init.

tests/test_gpu_pasta_sqrt.py runs the kernels on the same inputs.  Everything is compared exactly."""
import ctypes
import importlib.util
import os
import subprocess
import sys

import pytest

import pasta_sqrt_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import halo2_prover_amd
    return halo2_prover_amd.load()


def host(L, what, payload):
    cap = 3 * len(payload) + 64
    out = (ctypes.c_uint8 * cap)()
    n = ctypes.c_size_t(0)
    rc = L.h2_selftest_host(what, payload, len(payload), out, cap, ctypes.byref(n))
    return rc, bytes(out[:n.value])


def test_constants_file_is_what_the_tool_derives():
    spec = importlib.util.spec_from_file_location("pasta_sqrt_constants", os.path.join(ROOT, "tools", "pasta_sqrt_constants.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    with open(os.path.join(ROOT, "halo2_prover_amd", "csrc", "h2_pasta_sqrt_constants.inc")) as f:
        assert f.read() == tool.cpp_inc()
    for cid, (_, q) in zip((1, 2), tool.FIELDS):
        assert q == C.base_field(cid)
        z, g = tool.generator(q)
        assert g == C.generator(q) and pow(g, 1 << 31, q) == q - 1
        assert all(pow(y, (q - 1) // 2, q) == 1 for y in range(1, z))       # z is the smallest non-residue
        # the counts the header of csrc/h2_sqrt.hpp quotes, against the bit-by-bit constant-time form's 496 squarings
        c = tool.counts(q)
        assert c["log"][0] + c["log"][1] + c["root"][1] == 136 and c["total"] == (395 if cid == 1 else 393)


@pytest.mark.parametrize("cid", [0, 1, 2])
def test_host_square_root_matches_big_integers(lib, cid):
    xs = C.sqrt_inputs(cid)
    rc, out = host(lib, 11, bytes([cid]) + b"".join(x.to_bytes(32, "little") for x in xs))
    assert rc == 0 and len(out) == 33 * len(xs)
    seen = set()
    for i, a in enumerate(xs):
        root, status = int.from_bytes(out[33 * i:33 * i + 32], "little"), out[33 * i + 32]
        C.check_sqrt(cid, a, root, status)
        seen.add(status)
    assert seen == {0, 1, 3}


@pytest.mark.parametrize("cid", [1, 2])
def test_host_decompression_matches_transcript(lib, cid):
    words = C.decompress_mix(cid)
    rc, out = host(lib, 10, bytes([cid]) + b"".join(words))
    assert rc == 0 and len(out) == 65 * len(words)
    seen = set()
    for i, w in enumerate(words):
        got = (int.from_bytes(out[65 * i:65 * i + 32], "little"), int.from_bytes(out[65 * i + 32:65 * i + 64], "little"), out[65 * i + 64])
        assert got == C.expected_point(cid, w), (w.hex(), got)
        seen.add(got[2])
    assert seen == {0, 1, 2, 3}


def test_selftest_hooks_check_their_arguments(lib):
    assert host(lib, 10, bytes([0]) + bytes(32))[0] == -1                   # the Pasta wire form has no BN254 instantiation
    assert host(lib, 10, bytes([3]) + bytes(32))[0] == -1 and host(lib, 11, bytes([3]) + bytes(32))[0] == -1
    assert host(lib, 10, bytes([1]) + bytes(31))[0] == -1 and host(lib, 11, b"")[0] == -1
    # what = 8 stays BN254's: it takes no curve byte (a payload with one is H2_EINVAL: in_len % 32), and the Pasta encoding
    # of a point reads in BN254's wire form, bit 255 being the identity flag there
    assert host(lib, 8, bytes([1]) + bytes(32))[0] == -1
    assert host(lib, 8, (5 | (1 << 255)).to_bytes(32, "little")) == (0, bytes(64) + b"\x02")


NOT_INITIALISED = r"""
import sys
sys.path.insert(0, sys.argv[1])
import halo2_prover_amd
lib = halo2_prover_amd.load()
assert lib.h2_base_sqrt_device(1, None, 1, None, None, None) == -5
assert lib.h2_pasta_points_decompress_device(1, None, 1, None, None, None) == -5
assert lib.h2_ipa_challenge_products_sum_device(1, None, None, 4, 0, None, None) == -5
assert lib.h2_version() == 1002
print("not initialised: ok")
"""


def test_entry_points_fail_loudly_without_init():
    r = subprocess.run([sys.executable, "-c", NOT_INITIALISED, ROOT], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "not initialised: ok" in r.stdout, r.stdout + r.stderr


def test_symbols_and_wrappers_are_exported():
    import halo2_prover_amd
    from halo2_prover_amd import ipa
    for name in ("h2_base_sqrt_device", "h2_pasta_points_decompress_device", "h2_ipa_challenge_products_sum_device"):
        assert name in halo2_prover_amd.SYMBOLS
    assert callable(halo2_prover_amd.base_sqrt_device) and callable(halo2_prover_amd.pasta_points_decompress_device)
    assert callable(ipa.verify_proofs) and callable(ipa.challenge_products_sum)
    header = open(os.path.join(ROOT, "include", "h2hip.h")).read()
    for name in ("h2_base_sqrt_device", "h2_pasta_points_decompress_device", "h2_ipa_challenge_products_sum_device"):
        assert "int %s(" % name in header
