"""h2_generate_proofs without a GPU: it fails loudly before h2_init, and the Python layer exports it."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NOT_INITIALISED = r"""
import ctypes, os, sys
sys.path.insert(0, sys.argv[1])
import halo2_prover_amd
lib = halo2_prover_amd.load()
params = open(os.path.join(sys.argv[1], "tests", "golden", "params_k4.bin"), "rb").read()
jsons = (ctypes.c_char_p * 1)(b'{"x":6,"y":9,"constant":7,"z":2923}')
out = ctypes.create_string_buffer(b"\xab" * 4096, 4096)
lens = (ctypes.c_size_t * 1)(7)
total = ctypes.c_size_t(7)
rc = lib.h2_generate_proofs(params, len(params), 1, jsons, 1, None, None, out, 4096, lens, ctypes.byref(total))
assert (rc, lens[0], total.value, out.raw) == (-5, 7, 7, b"\xab" * 4096), (rc, lens[0], total.value)
rc = lib.h2_generate_proofs(params, len(params), 0, None, 1, None, None, None, 0, None, ctypes.byref(total))
assert (rc, total.value) == (-5, 7), (rc, total.value)
assert lib.h2_version() == 1002
print("not initialised: ok")
"""


def test_batch_proving_fails_loudly_without_init():
    """no CPU fallback: without h2_init the batch prover returns H2_ENOTINIT, for count = 1 and count = 0, and writes
    nothing (a process of its own, so that it holds whether or not another test has initialised the library)"""
    r = subprocess.run([sys.executable, "-c", NOT_INITIALISED, ROOT], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "not initialised: ok" in r.stdout, r.stdout + r.stderr


def test_python_wrapper_and_symbols_are_exported():
    import halo2_prover_amd
    assert callable(halo2_prover_amd.generate_proofs)
    for name in ("h2_generate_proofs", "h2_selftest_commit_launches", "h2_selftest_set_prove_group"):
        assert name in halo2_prover_amd.SYMBOLS, name
