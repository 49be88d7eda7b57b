"""CPU (no GPU): the ABI of the table-free MSM -- h2_msm_points_device, h2_msm_points, h2_msm_points_plan and the two
test hooks that go with them -- and what can be said about its launches on the host: the window geometry for every
curve and size, the route a size takes, and the bounds proof of the launch sequence (DESIGN.md sections 4.1 and 4.4)
for a sweep of shapes sampled as tests/test_msm_geometry.py samples the resident-table MSM's."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = {"h2_msm_points_device": 8, "h2_msm_points": 5, "h2_msm_points_plan": 3}
HOOKS = {"h2_selftest_msm_points_check": 6, "h2_selftest_set_msm_points_small_max": 1}
NBITS = {0: 254, 1: 255, 2: 255}
SIZE_MAX = ctypes.c_size_t(-1).value


@pytest.fixture(scope="module")
def lib():
    import halo2_prover_amd
    return halo2_prover_amd.load()


def plan(lib, curve, n):
    import halo2_prover_amd
    p = halo2_prover_amd.lib.MsmPointsPlan()
    st = lib.h2_msm_points_plan(curve, n, ctypes.byref(p))
    return st, p


def check(lib, curve, n, m, stride=None, guard=0):
    out = (ctypes.c_uint64 * 8)()
    st = lib.h2_selftest_msm_points_check(curve, n, m, n if stride is None else stride, guard, out)
    return st, dict(zip(("c", "W", "B", "tile", "lds", "group", "T", "regions"), [int(x) for x in out]))


def test_library_exports_the_entry_points_and_hooks(lib):
    for name in list(ENTRY) + list(HOOKS):
        assert hasattr(lib, name), name
    assert lib.h2_version() == 1002


def test_loader_lists_them_with_their_arguments():
    import halo2_prover_amd
    I, P, Z = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
    S = halo2_prover_amd.SYMBOLS
    # curve, d_points, d_scalars, n, col_stride, m, d_out_jac, stream
    assert S["h2_msm_points_device"] == (I, [I, P, P, Z, Z, Z, P, P])
    # curve, points, scalars, n, out_jac
    assert S["h2_msm_points"] == (I, [I, P, P, Z, P])
    res, args = S["h2_msm_points_plan"]
    assert res is I and args[:2] == [I, Z] and len(args) == 3
    # curve, n, m, col_stride, guard, out
    assert S["h2_selftest_msm_points_check"] == (I, [I, Z, Z, Z, I, P])
    assert S["h2_selftest_set_msm_points_small_max"] == (I, [Z])


def test_headers_declare_them():
    text = open(os.path.join(ROOT, "include", "h2hip.h")).read()
    for name, argc in ENTRY.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, "include/h2hip.h does not declare " + name
        assert len(m.group(1).split(",")) == argc, name
    assert "h2_msm_points_plan_t" in text
    text = open(os.path.join(ROOT, "include", "h2hip_selftest.h")).read()
    for name, argc in HOOKS.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, "include/h2hip_selftest.h does not declare " + name
        assert len(m.group(1).split(",")) == argc, name


def test_they_fail_loudly_without_init(lib):
    """no CPU fallback: before h2_init a call is H2_ENOTINIT (H2_EINVAL's null pointers if another test of this process
    has initialised a device)"""
    out = (ctypes.c_uint64 * 12)()
    assert lib.h2_msm_points_device(0, None, None, 8, 8, 1, None, None) in (-5, -1)
    assert lib.h2_msm_points(0, None, None, 8, out) in (-5, -1)


def sizes():
    s = {1, 2, 3}
    for k in range(1, 25):
        s |= {(1 << k) - 1, 1 << k, (1 << k) + 1}
    return sorted(x for x in s if 1 <= x <= (1 << 24) + 1)


@pytest.mark.parametrize("curve", [0, 1, 2])
def test_plan_geometry_covers_the_scalar_at_every_size(lib, curve):
    """the windows are consecutive and cover nbits + 1 bits (the spare bit keeps the top window from carrying out), the
    widest is c, and the W * B words of histogram fit the LDS the sort front may use"""
    for n in sizes():
        st, p = plan(lib, curve, n)
        assert st == 0, n
        W = p.windows
        widths, offs = list(p.width[:W]), list(p.offset[:W])
        assert p.scalar_bits == NBITS[curve]
        assert sum(widths) == NBITS[curve] + 1, n
        assert 1 <= W <= 48 and max(widths) == p.window_bits and min(widths) >= p.window_bits - 1, n
        assert offs == [sum(widths[:w]) for w in range(W)], n
        assert p.buckets == 1 << (p.window_bits - 1), n
        assert p.lds_bytes == W * p.buckets * 4 and p.lds_bytes <= p.lds_limit <= 160 * 1024, n
        assert p.max_n >= 1 << 24


def test_plan_reports_the_route_and_follows_the_hook(lib):
    st, p = plan(lib, 0, 1)
    X = p.crossover
    assert st == 0 and 1 < X < (1 << 20)
    for n in (0, 1, X - 1):
        assert plan(lib, 0, n)[1].route == 0, n
    for n in (X, X + 1, 1 << 16, 1 << 24):
        assert plan(lib, 0, n)[1].route == 1, n
    try:
        assert lib.h2_selftest_set_msm_points_small_max(0) == 0       # every input takes buckets
        assert [plan(lib, 0, n)[1].route for n in (1, 2, 65)] == [1, 1, 1]
        assert lib.h2_selftest_set_msm_points_small_max(100) == 0
        assert [plan(lib, 0, n)[1].route for n in (99, 100)] == [0, 1]
        assert plan(lib, 0, 1)[1].crossover == 100
    finally:
        lib.h2_selftest_set_msm_points_small_max(SIZE_MAX)
    assert plan(lib, 0, 1)[1].crossover == X


def test_plan_refuses_bad_arguments(lib):
    import halo2_prover_amd
    p = halo2_prover_amd.lib.MsmPointsPlan()
    assert lib.h2_msm_points_plan(9, 16, ctypes.byref(p)) == -1
    assert lib.h2_msm_points_plan(0, 16, None) == -1
    st, q = plan(lib, 0, 16)
    assert lib.h2_msm_points_plan(0, q.max_n + 1, ctypes.byref(p)) == -1
    assert lib.h2_msm_points_plan(0, q.max_n, ctypes.byref(p)) == 0


@pytest.mark.parametrize("curve", [0, 1, 2])
def test_every_shape_passes_the_bounds_proof(lib, curve):
    shapes = 0
    for k in range(0, 25):
        for n in {1 << k, (1 << k) - 1, (1 << k) + 1, 3 * (1 << k) // 2 + 1}:
            if n < 1 or n > (1 << 24) + 1:
                continue
            for m in (1, 2, 3, 5, 7, 16, 70):
                for stride in (n, n + 7):
                    st, info = check(lib, curve, n, m, stride)
                    assert st == 0, (n, m, stride, lib.h2_last_device_error())
                    assert 1 <= info["group"] <= m and info["lds"] == info["W"] * info["B"] * 4
                    # a group's sorted entries are indexed with 31 bits: wider batches run in column groups
                    assert info["group"] * info["W"] * n < (1 << 31)
                    st, g = check(lib, curve, n, m, stride, guard=1)
                    assert st == 0, (n, m, stride, "guard", lib.h2_last_device_error())
                    assert g["regions"] == info["regions"]
                    shapes += 1
    assert shapes > 1000


def test_plan_and_proof_agree_on_the_geometry(lib):
    for n in (1, 1000, 1 << 13, 1 << 16, 1 << 20, 1 << 24):
        _, p = plan(lib, 0, n)
        _, info = check(lib, 0, n, 1)
        assert (info["c"], info["W"], info["B"]) == (p.window_bits, p.windows, p.buckets), n


def test_bad_strides_and_lengths_are_refused(lib):
    assert check(lib, 0, 1 << 12, 3, stride=(1 << 12) - 1)[0] == -1       # columns would overlap
    assert b"col_stride" in lib.h2_last_device_error()
    assert check(lib, 0, 1 << 12, 1, stride=(1 << 12) - 1)[0] == -1       # one column too: the ABI asks col_stride >= n
    assert check(lib, 0, 0, 1)[0] == -1
    assert check(lib, 0, 16, 0)[0] == -1
    assert check(lib, 9, 16, 1)[0] == -1
    assert check(lib, 0, (1 << 26) + 1, 1)[0] == -1
