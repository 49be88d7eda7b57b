"""CPU (no GPU): the ABI of h2_extended_to_coeff_device -- exported by the built library, listed by the Python loader
with its thirteen arguments, declared in include/h2hip.h; h2_version() did not move (a host detects the entry point by
its symbol)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "h2_extended_to_coeff_device"


def test_library_exports_the_entry_point():
    import halo2_prover_amd
    lib = halo2_prover_amd.load()
    assert hasattr(lib, NAME)
    assert lib.h2_version() == 1002


def test_loader_lists_it_with_thirteen_arguments():
    import halo2_prover_amd
    res, args = halo2_prover_amd.SYMBOLS[NAME]
    assert res is ctypes.c_int and len(args) == 13
    # curve, d_ext, ext_log_n, m, ext_omega_inv, scale, zeta_inv, d_t, t_period, d_out, out_len, out_stride, stream
    assert args == [ctypes.c_int, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p,
                    ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t,
                    ctypes.c_void_p]


def test_header_declares_it():
    text = open(os.path.join(ROOT, "include", "h2hip.h")).read()
    m = re.search(r"\bint\s+" + NAME + r"\s*\(([^)]*)\)\s*;", text)
    assert m, "include/h2hip.h does not declare " + NAME
    assert len(m.group(1).split(",")) == 13


def test_it_fails_loudly_without_init():
    """no CPU fallback: before h2_init the call is H2_ENOTINIT (H2_EINVAL's null pointers if another test of this
    process has initialised a device)"""
    import halo2_prover_amd
    lib = halo2_prover_amd.load()
    z = (ctypes.c_uint64 * 4)(1, 0, 0, 0)
    assert lib.h2_extended_to_coeff_device(0, None, 6, 1, z, z, z, None, 0, None, 48, 48, None) in (-5, -1)
