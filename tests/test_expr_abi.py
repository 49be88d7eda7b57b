"""CPU (no GPU): the ABI of h2_expr_compile / h2_expr_release / h2_expr_info / h2_expr_dump / h2_expr_eval_device --
exported by the built library, listed by the Python loader with their argument lists, declared in include/h2hip.h;
h2_version() did not move (a host detects the entry points by their symbols); compile, info, dump and release are host
only and work before h2_init; every rule of h2_expr_compile's H2_EINVAL is hit once and named in the error text."""
import ctypes
import os
import re
import struct

import pytest

import test_expr_program as T
from test_expr_public import (ADD, COL, CONST, EHANDLE, EINVAL, FIELDS, MUL, VAR, compile_public, dump, info, mont_words)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_P, _Z, _I, _U32, _U64 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint64
ARGS = {
    # curve, nodes, n_nodes, consts, n_consts, n_cols, n_vars, handle_out
    "h2_expr_compile": [_I, _P, _Z, _P, _Z, _U32, _U32, ctypes.POINTER(_U64)],
    "h2_expr_release": [_U64],
    "h2_expr_info": None,                            # handle, out (a pointer to the loader's ExprInfo)
    "h2_expr_dump": [_U64, _P, _Z, ctypes.POINTER(_Z)],
    # handle, d_cols, log_len, vars, m, log_rows, rot_step, d_out, out_stride, stream
    "h2_expr_eval_device": [_U64, _P, _P, _P, _Z, _U32, _U32, _P, _Z, _P],
}
COUNTS = {"h2_expr_compile": 8, "h2_expr_release": 1, "h2_expr_info": 2, "h2_expr_dump": 4, "h2_expr_eval_device": 10}


@pytest.fixture(scope="module")
def lib():
    import halo2_prover_amd
    return halo2_prover_amd.load()


@pytest.mark.parametrize("name", sorted(ARGS))
def test_library_exports_the_entry_point(lib, name):
    assert hasattr(lib, name)
    assert lib.h2_version() == 1002


@pytest.mark.parametrize("name", sorted(ARGS))
def test_loader_lists_it_with_its_arguments(name):
    import halo2_prover_amd
    res, args = halo2_prover_amd.SYMBOLS[name]
    assert res is ctypes.c_int and len(args) == COUNTS[name]
    if ARGS[name] is None:
        assert args == [_U64, ctypes.POINTER(halo2_prover_amd.lib.ExprInfo)]
    else:
        assert args == ARGS[name]


@pytest.mark.parametrize("name", sorted(ARGS))
def test_header_declares_it(name):
    text = open(os.path.join(ROOT, "include", "h2hip.h")).read()
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, "include/h2hip.h does not declare " + name
    assert len(m.group(1).split(",")) == COUNTS[name]
    assert "h2_expr_node_t;" in text and "h2_expr_info_t;" in text


def test_the_info_struct_matches_the_header():
    import halo2_prover_amd.lib as L
    assert ctypes.sizeof(L.ExprInfo) == 48
    assert [n for n, _ in L.ExprInfo._fields_] == ["curve", "instructions", "products", "column_reads", "slots", "constants",
                                                   "reductions", "n_cols", "n_vars", "lds_bytes", "min_rot", "max_rot"]


def test_compile_info_dump_and_release_need_no_init(lib):
    """host only: these run on a machine without a GPU, whether or not another test of the process initialised one"""
    nodes = [(COL, 0, 0, 1), (VAR, 0, 0, 0), (MUL, 0, 1, 0), (CONST, 0, 0, 0), (ADD, 2, 3, 0)]
    for curve, p in FIELDS.items():
        rc, h = compile_public(lib, curve, nodes, [p - 1], 1, 1)
        assert rc == 0 and h != 0
        i = info(lib, h)
        assert (i.curve, i.instructions, i.products, i.column_reads, i.n_cols, i.n_vars) == (curve, 2, 1, 1, 1, 1)
        prog = dump(lib, h, 1)
        assert sorted(prog["table"]) == [0, 1, p - 1] and prog["table"][prog["var_slot"][0]] == 0
        assert lib.h2_expr_release(h) == 0


def test_eval_fails_loudly_without_init(lib):
    """no CPU fallback: before h2_init the call is H2_ENOTINIT (H2_EINVAL's null pointers if another test of this process
    has initialised a device)"""
    rc, h = compile_public(lib, 0, [(COL, 0, 0, 0)], [], 1, 0)
    assert rc == 0
    assert lib.h2_expr_eval_device(h, None, None, None, 1, 4, 1, None, 16, None) in (-5, -1)
    assert lib.h2_expr_release(h) == 0


def live_dag_limits(lib, curve):
    """-> (the largest live_dag the compiler takes, its slots)"""
    last = None
    for n in range(60, 200):
        nodes = T.live_dag(n)
        rc, h = compile_public(lib, curve, nodes, [], n + 1, 0)
        if rc != 0:
            assert rc == EINVAL
            return n, last
        last = info(lib, h).slots
        assert lib.h2_expr_release(h) == 0
    raise AssertionError("no live_dag is refused")


def test_every_rule_of_compile(lib):
    col, col1 = (COL, 0, 0, 0), (COL, 1, 0, 0)
    ok = [col, col1, (ADD, 0, 1, 0)]
    h = ctypes.c_uint64(0)
    raw = b"".join(struct.pack("<4i", *nd) for nd in ok)
    one = mont_words([1], FIELDS[0])

    def err():
        return lib.h2_last_device_error().decode()

    assert lib.h2_expr_compile(3, raw, 3, None, 0, 2, 0, ctypes.byref(h)) == EINVAL and "curve" in err()
    assert lib.h2_expr_compile(0, None, 3, None, 0, 2, 0, ctypes.byref(h)) == EINVAL and "null" in err()
    assert lib.h2_expr_compile(0, raw, 3, None, 1, 2, 0, ctypes.byref(h)) == EINVAL and "null" in err()
    assert lib.h2_expr_compile(0, raw, 3, None, 0, 2, 0, None) == EINVAL and "null" in err()
    assert lib.h2_expr_compile(0, raw, 0, None, 0, 2, 0, ctypes.byref(h)) == EINVAL and "n_nodes" in err()
    assert lib.h2_expr_compile(0, raw, (1 << 20) + 1, None, 0, 2, 0, ctypes.byref(h)) == EINVAL and "n_nodes" in err()
    assert lib.h2_expr_compile(0, raw, 3, one, (1 << 20) + 1, 2, 0, ctypes.byref(h)) == EINVAL and "n_consts" in err()
    assert lib.h2_expr_compile(0, raw, 3, None, 0, 2, (1 << 20) + 1, ctypes.byref(h)) == EINVAL and "n_vars" in err()
    assert lib.h2_expr_compile(0, raw, 3, None, 0, (1 << 22) + 1, 0, ctypes.byref(h)) == EINVAL and "n_cols" in err()
    bad = {
        "earlier node": [col, col1, (ADD, 0, 3, 0), (ADD, 0, 2, 0)],
        "earlier node ": [col, (MUL, 0, 1, 0)],
        "earlier node  ": [col, (MUL, -1, 0, 0)],
        "unknown op": [col, col1, (6, 0, 1, 0)],
        "unknown op ": [col, col1, (-1, 0, 1, 0)],
        "no such constant": [col, (CONST, 0, 0, 1), (ADD, 0, 1, 0)],
        "no such constant ": [col, (CONST, 0, 0, -1), (ADD, 0, 1, 0)],
        "no such column": [col, (COL, 2, 0, 0), (ADD, 0, 1, 0)],
        "no such variable": [col, (VAR, 0, 0, 1), (ADD, 0, 1, 0)],
        "no such variable ": [col, (VAR, 0, 0, -1), (ADD, 0, 1, 0)],
        "rotation": [(COL, 0, 0, 128), col, (ADD, 0, 1, 0)],
        "rotation ": [(COL, 0, 0, -129), col, (ADD, 0, 1, 0)],
        "column index": [(COL, -1, 0, 0), col, (ADD, 0, 1, 0)],
    }
    for rule, nodes in bad.items():
        assert compile_public(lib, 0, nodes, [7], 2, 1)[0] == EINVAL, rule
        assert rule.strip() in err(), (rule, err())
    # the edges that are fine: rotations -128 and 127, column 2^22 - 1, 2^20 nodes' worth of indices is not needed here
    rc, hh = compile_public(lib, 0, [(COL, (1 << 22) - 1, 0, -128), (COL, 0, 0, 127), (MUL, 0, 1, 0)], [], 1 << 22, 0)
    assert rc == 0 and lib.h2_expr_release(hh) == 0
    for curve, p in FIELDS.items():                                     # a constant that is not canonical
        assert compile_public(lib, curve, [col, (CONST, 0, 0, 0), (ADD, 0, 1, 0)], [p], 1, 0)[0] == EINVAL
        assert "canonical" in err()
    # live values: 75 fit the 160 KiB of LDS one workgroup may hold, the first DAG past that is refused
    n, slots = live_dag_limits(lib, 1)
    assert slots == 75 and "live values" in err()
    assert max(1, slots - 4) * T.SLOT_BYTES <= T.LDS_MAX < max(1, slots + 1 - 4) * T.SLOT_BYTES


def test_a_fold_as_deep_as_the_limit_compiles_on_a_small_stack(lib):
    """h = h * y + gate_i over 2^19 - 1 gates: 2^20 nodes, every one on one chain, compiled on a thread with 256 KiB of
    stack (a Rust std::thread has 2 MiB).  The compiler does not recurse, so the depth of a DAG costs no stack."""
    import threading
    import numpy as np
    steps = (1 << 19) - 1
    nd = np.zeros((1 << 20, 4), dtype=np.int32)
    nd[0] = (COL, 0, 0, 0)
    nd[1] = (VAR, 0, 0, 0)
    k = 2 + 2 * np.arange(steps, dtype=np.int32)          # node k = h * y, node k + 1 = that + the gate column
    nd[k] = np.stack([np.full(steps, MUL), np.where(k == 2, 0, k - 1), np.full(steps, 1), np.zeros(steps)], axis=1)
    nd[k + 1] = np.stack([np.full(steps, ADD), k, np.zeros(steps), np.zeros(steps)], axis=1)
    raw = nd.tobytes()
    result = {}

    def work():
        h = ctypes.c_uint64(0)
        result["rc"] = lib.h2_expr_compile(1, raw, 1 << 20, None, 0, 1, 1, ctypes.byref(h))
        result["h"] = h.value

    old = threading.stack_size(256 * 1024)
    try:
        t = threading.Thread(target=work)
        t.start()
        t.join()
    finally:
        threading.stack_size(old)
    assert result["rc"] == 0
    i = info(lib, result["h"])
    # every step is one product and one sum; the sums of a running value and a column stay small: few reductions
    assert i.products >= steps and i.instructions == 2 * steps + i.reductions and i.slots == 1
    assert lib.h2_expr_release(result["h"]) == 0


def test_a_released_or_unknown_handle(lib):
    rc, h = compile_public(lib, 2, [(COL, 0, 0, 0)], [], 1, 0)
    assert rc == 0 and lib.h2_expr_release(h) == 0
    import halo2_prover_amd.lib as L
    n = ctypes.c_size_t(0)
    buf = ctypes.create_string_buffer(64)
    for bad in (h, 0, 1 << 60):
        assert lib.h2_expr_release(bad) == EHANDLE
        assert lib.h2_expr_info(bad, ctypes.byref(L.ExprInfo())) == EHANDLE
        assert lib.h2_expr_dump(bad, buf, 64, ctypes.byref(n)) == EHANDLE
        assert lib.h2_expr_eval_device(bad, None, None, None, 1, 4, 1, None, 16, None) in (EHANDLE, -5)


def test_the_python_class_is_exported():
    import halo2_prover_amd
    prog = halo2_prover_amd.ExprProgram([(COL, 0, 0, 0), (VAR, 0, 0, 0), (MUL, 0, 1, 0)], [], 1, 1, "vesta")
    assert prog.info()["instructions"] == 1 and prog.info()["curve"] == 2
    assert len(prog.dump()) == 24 + 12 + 2 * 32 + 4
    prog.release()
    for name in ("info", "dump", "release", "eval"):
        assert callable(getattr(halo2_prover_amd.ExprProgram, name))
