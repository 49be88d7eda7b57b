"""GPU: the table-free MSM (h2_msm_points_device / h2_msm_points) against the CPU oracle, after affine normalisation.

Both routes -- double-and-add below the crossover, buckets from it -- at the sizes around every change of path, ragged
column strides whose sort grid has surplus blocks, scalars on every window boundary of the plan,
exceptional points, hot buckets, the scratch shared with the resident-table MSM, red zones behind every region of the
arena, two streams, the host form and the error codes.  No point passed here is off the curve.
"""
import ctypes

import numpy as np
import pytest

import oracle_lib as O
import pyref as R

pytestmark = pytest.mark.gpu

CURVES = ["bn254", "pallas", "vesta"]
CID = O.CURVE_IDS
SEED = 0x48324D5300000000
SIZE_MAX = ctypes.c_size_t(-1).value


def scalars(curve, n, seed):
    return O.synth_scalars(O.CURVE_SCALAR_FIELD[CID[curve]], SEED | seed, n).reshape(n, 4)


_bases = {}


def bases_of(curve, n, seed=0xB5):
    """the first n of one vector of points per (curve, seed), generated once"""
    key = (curve, seed)
    if key not in _bases or _bases[key].shape[0] < n:
        _bases[key] = O.synth_bases(CID[curve], SEED | seed, max(n, 1 << 14), threads=8).reshape(-1, 8)
    return _bases[key][:n].copy()


def mont(curve, x):
    f = R.CURVES[curve].scalar
    return np.array(f.limbs(x % f.p), dtype=np.uint64)


def neg_point(curve, p):
    q = p.copy()
    q[4:] = O.field_op(O.CURVE_BASE_FIELD[CID[curve]], "neg", p[4:])
    return q


def want_of(curve, col, pts):
    if col.shape[0] == 0:
        return np.zeros(8, dtype=np.uint64)
    return O.to_affine(CID[curve], O.best_multiexp(CID[curve], col, pts, threads=8))


def plan_of(lib, curve, n):
    import halo2_prover_amd
    p = halo2_prover_amd.lib.MsmPointsPlan()
    assert lib.h2_msm_points_plan(CID[curve], n, ctypes.byref(p)) == 0
    return p


def run_device(lib, curve, pts, cols, stride=None, stream=None, sync=True):
    """cols: list of (n, 4) columns -> (m, 12) raw Jacobian results"""
    import torch
    m, n = len(cols), pts.shape[0]
    stride = n if stride is None else stride
    buf = np.zeros((m, max(stride, 1), 4), dtype=np.uint64)
    for j, c in enumerate(cols):
        buf[j, :n] = c
    d_s = torch.from_numpy(buf.view(np.int64)).cuda()
    d_p = torch.from_numpy(np.ascontiguousarray(pts if n else np.zeros((1, 8), dtype=np.uint64)).view(np.int64)).cuda()
    d_o = torch.full((max(m, 1), 12), 0x5A5A5A5A, dtype=torch.int64, device="cuda")
    st = lib.h2_msm_points_device(CID[curve], ctypes.c_void_p(d_p.data_ptr()), ctypes.c_void_p(d_s.data_ptr()), n, stride, m,
                                  ctypes.c_void_p(d_o.data_ptr()), ctypes.c_void_p(stream or 0))
    assert st == 0, (st, lib.h2_last_device_error())
    if not sync:
        return d_o, (d_s, d_p)
    torch.cuda.synchronize()
    return d_o.cpu().numpy().view(np.uint64)[:m]


def check_cols(lib, curve, pts, cols, stride=None):
    got = run_device(lib, curve, pts, cols, stride)
    for j, c in enumerate(cols):
        assert np.array_equal(O.to_affine(CID[curve], got[j]), want_of(curve, c, pts)), (curve, pts.shape[0], len(cols), j)
    return got


@pytest.fixture()
def buckets_everywhere(h2):
    lib = h2.load()
    try:
        lib.h2_selftest_set_msm_points_small_max(0)
        yield lib
    finally:
        lib.h2_selftest_set_msm_points_small_max(SIZE_MAX)


def guard_report(lib):
    out = (ctypes.c_uint64 * 2)()
    first = ctypes.create_string_buffer(256)
    assert lib.h2_selftest_msm_guard_report(out, first, 256) == 0
    return int(out[0]), int(out[1]), first.value.decode()


@pytest.fixture()
def guarded(h2):
    lib = h2.load()
    try:
        lib.h2_selftest_msm_guard(1)
        yield lib
    finally:
        lib.h2_selftest_msm_guard(0)


# ---------------------------------------------------------------------------------- sizes ----
@pytest.mark.parametrize("curve", CURVES)
def test_every_size_on_both_routes(h2, curve):
    lib = h2.load()
    X = int(plan_of(lib, curve, 1).crossover)
    sizes = sorted({0, 1, 2, 3, 63, 64, 65, X - 1, X, X + 1, 1000, 4097, (1 << 14) + 1})
    for n in sizes:
        assert plan_of(lib, curve, n).route == (0 if n < X else 1)
        check_cols(lib, curve, bases_of(curve, n), [scalars(curve, n, 0x100 + n % 251)])
    try:
        lib.h2_selftest_set_msm_points_small_max(0)
        for n in [s for s in sizes if s < X]:
            if n:
                assert plan_of(lib, curve, n).route == 1
            check_cols(lib, curve, bases_of(curve, n), [scalars(curve, n, 0x100 + n % 251)])
    finally:
        lib.h2_selftest_set_msm_points_small_max(SIZE_MAX)


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("m", [3, 5])
def test_columns_with_a_ragged_stride(h2, curve, m):
    """n = 1000: two tiles per column, so the sort grid of 6 resp. 10 blocks is rounded up to 8 resp. 16 -- the surplus
    blocks of section 4.4"""
    lib = h2.load()
    n = 1000
    cols = [scalars(curve, n, 0x200 + j) for j in range(m)]
    cols[1][n // 2:] = 0
    check_cols(lib, curve, bases_of(curve, n), cols, stride=n + 7)


# --------------------------------------------------------------------------- edge scalars ----
def edge_scalars(curve, p):
    r = R.CURVES[curve].scalar.p
    W = p.windows
    off, width = list(p.offset[:W]), list(p.width[:W])
    e = [0, 1, 2, r - 1, r - 2, (r - 1) // 2]
    for w in range(W):
        e += [(1 << off[w]) - 1, 1 << off[w], (1 << off[w]) + 1]
    for w in (0, 1, W // 2, W - 2):                       # the sign tie: |d| = 2^(width - 1) stays positive, one more turns
        e += [(1 << (width[w] - 1)) << off[w], ((1 << (width[w] - 1)) + 1) << off[w]]
    e += [1 << off[W - 1], 3 << off[W - 1]]               # the only non-zero digit is the top window's
    return [x % r for x in e]


@pytest.mark.parametrize("curve", CURVES)
def test_edge_scalars_through_the_bucket_route(h2, buckets_everywhere, curve):
    """one column per edge scalar (that scalar against its own point, zeros elsewhere: an error cannot hide in a sum,
    and all but a few window results go into the combine as identities), then all of them in one column"""
    lib = buckets_everywhere
    n = 256
    p = plan_of(lib, curve, n)
    edges = edge_scalars(curve, p)
    assert len(edges) <= n and p.route == 1
    pts = bases_of(curve, n)
    assert len({bytes(x) for x in pts}) == n            # distinct points
    cols = []
    for j, x in enumerate(edges):
        c = np.zeros((n, 4), dtype=np.uint64)
        c[j] = mont(curve, x)
        cols.append(c)
    both = scalars(curve, n, 0x333)
    for j, x in enumerate(edges):
        both[j] = mont(curve, x)
    cols.append(both)
    got = run_device(lib, curve, pts, cols)
    for j, x in enumerate(edges):
        want = O.to_affine(CID[curve], O.scalar_mul(CID[curve], mont(curve, x), pts[j]))
        assert np.array_equal(O.to_affine(CID[curve], got[j]), want), (curve, j, hex(x))
    assert not got[0][8:].any()                            # 0 * P: the identity leaves as z = 0
    assert np.array_equal(O.to_affine(CID[curve], got[-1]), want_of(curve, both, pts))


# ------------------------------------------------------------------------- special points ----
@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("route", ["small", "buckets"])
def test_special_points(h2, curve, route):
    lib = h2.load()
    n = 200
    try:
        lib.h2_selftest_set_msm_points_small_max(0 if route == "buckets" else 1 << 20)
        pts = bases_of(curve, n)
        # identities among the bases
        a = pts.copy()
        a[[0, 7, 64, n - 1]] = 0
        check_cols(lib, curve, a, [scalars(curve, n, 0x400), scalars(curve, n, 0x401)])
        # one point repeated with equal scalars: doublings inside a bucket
        b = pts.copy()
        b[10:20] = pts[3]
        s = scalars(curve, n, 0x402)
        s[10:20] = s[3]
        check_cols(lib, curve, b, [s])
        # P and -P with equal scalars, nothing else: the identity, z = 0
        c = np.zeros((n, 8), dtype=np.uint64)
        t = np.zeros((n, 4), dtype=np.uint64)
        for i in range(0, 40, 2):
            c[i], c[i + 1] = pts[i], neg_point(curve, pts[i])
            t[i] = t[i + 1] = scalars(curve, 1, 0x410 + i)[0]
        got = check_cols(lib, curve, c, [t, scalars(curve, n, 0x403)])
        assert not got[0][8:].any()
        # all scalars zero
        got = check_cols(lib, curve, pts, [np.zeros((n, 4), dtype=np.uint64)])
        assert not got[0][8:].any()
    finally:
        lib.h2_selftest_set_msm_points_small_max(SIZE_MAX)


def test_hot_buckets(h2):
    """every scalar equal: each window has ONE bucket of 2^16 entries, cut into more pieces than the hot-task path's
    threshold (MSM_HOT_SPAN = 256 pieces)"""
    lib = h2.load()
    curve, n = "bn254", 1 << 16
    out = (ctypes.c_uint64 * 8)()
    assert lib.h2_selftest_msm_points_check(CID[curve], n, 1, n, 0, out) == 0
    assert n // int(out[6]) > 256                          # pieces of a window's one bucket = n / entries per thread
    pts = bases_of(curve, n, seed=0xB7)
    col = np.tile(scalars(curve, 1, 0x500), (n, 1))
    check_cols(lib, curve, pts, [col])


# ---------------------------------------------------------------------- workspace sharing ----
def sharing_sequence(h2, lib, curve="bn254"):
    """a registered MSM, a table-free one, the registered one again, a table-free one -- one stream, one workspace: the
    counter region a launch sequence leaves zero is taken on trust by the next one, of either kind"""
    import torch
    b12 = bases_of(curve, 1 << 12, seed=0xC1)
    reg = h2.Bases(curve, b12)
    try:
        def registered(n, m, seed):
            cols = np.stack([scalars(curve, n, seed + j) for j in range(m)])
            d = torch.from_numpy(cols.view(np.int64)).cuda()
            out = torch.zeros((m, 12), dtype=torch.int64, device="cuda")
            reg.msm_device(d.data_ptr(), n, m, out.data_ptr())
            torch.cuda.synchronize()
            res = out.cpu().numpy().view(np.uint64)
            for j in range(m):
                assert np.array_equal(O.to_affine(CID[curve], res[j]), want_of(curve, cols[j], b12[:n])), ("registered", n, m, j)

        registered(1 << 12, 3, 0x600)
        check_cols(lib, curve, bases_of(curve, 1000), [scalars(curve, 1000, 0x610 + j) for j in range(5)])
        registered(1 << 10, 1, 0x620)
        check_cols(lib, curve, bases_of(curve, 4097), [scalars(curve, 4097, 0x630)])
    finally:
        reg.release()


def test_workspace_shared_with_the_registered_msm(h2):
    sharing_sequence(h2, h2.load())


# ------------------------------------------------------------------------------ guard mode ----
def test_red_zones_stay_intact(h2, guarded):
    lib = guarded
    for curve, m in (("bn254", 3), ("pallas", 5)):
        n = 1000
        cols = [scalars(curve, n, 0x700 + j) for j in range(m)]
        cols[1][n // 2:] = 0
        check_cols(lib, curve, bases_of(curve, n), cols, stride=n + 7)
    check_cols(lib, "bn254", bases_of("bn254", 4097), [scalars("bn254", 4097, 0x710)])
    launches, violations, first = guard_report(lib)
    assert launches == 3 and violations == 0, first
    sharing_sequence(h2, lib)
    launches, violations, first = guard_report(lib)
    assert launches == 7 and violations == 0, first


# ----------------------------------------------------------------------------- two streams ----
def test_two_streams_at_once(h2):
    import torch
    lib = h2.load()
    curve = "bn254"
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    p1, p2 = bases_of(curve, 4097), bases_of(curve, 3000, seed=0xB9)
    c1 = [scalars(curve, 4097, 0x800 + j) for j in range(2)]
    c2 = [scalars(curve, 3000, 0x810 + j) for j in range(3)]
    o1, keep1 = run_device(lib, curve, p1, c1, stream=s1.cuda_stream, sync=False)
    o2, keep2 = run_device(lib, curve, p2, c2, stream=s2.cuda_stream, sync=False)
    o3, keep3 = run_device(lib, curve, p1, c1[::-1], stream=s1.cuda_stream, sync=False)
    torch.cuda.synchronize()
    r1, r2, r3 = (o.cpu().numpy().view(np.uint64) for o in (o1, o2, o3))
    for j in range(2):
        assert np.array_equal(O.to_affine(CID[curve], r1[j]), want_of(curve, c1[j], p1)), j
        assert np.array_equal(O.to_affine(CID[curve], r3[1 - j]), want_of(curve, c1[j], p1)), j
    for j in range(3):
        assert np.array_equal(O.to_affine(CID[curve], r2[j]), want_of(curve, c2[j], p2)), j


# ------------------------------------------------------------------------------- host form ----
@pytest.mark.parametrize("n", [65, 4097])
def test_host_form_equals_the_device_form(h2, n):
    lib = h2.load()
    curve = "bn254"
    pts, col = bases_of(curve, n), scalars(curve, n, 0x900 + n % 7)
    dev = run_device(lib, curve, pts, [col])[0]
    host = h2.api.msm_points(col, pts, curve)
    assert np.array_equal(O.to_affine(CID[curve], host), O.to_affine(CID[curve], dev))
    assert np.array_equal(O.to_affine(CID[curve], host), want_of(curve, col, pts))


def test_host_form_shape_checks(h2):
    with pytest.raises(ValueError):
        h2.api.msm_points(np.zeros((3, 4), dtype=np.uint64), np.zeros((4, 8), dtype=np.uint64))
    assert not h2.api.msm_points(np.zeros((0, 4), dtype=np.uint64), np.zeros((0, 8), dtype=np.uint64)).any()


# ----------------------------------------------------------------------------- error codes ----
def test_error_codes(h2):
    import torch
    lib = h2.load()
    n = 16
    d_p = torch.from_numpy(bases_of("bn254", n).view(np.int64)).cuda()
    d_s = torch.from_numpy(np.tile(scalars("bn254", n, 0xA00), (2, 1)).view(np.int64)).cuda()
    d_o = torch.full((3, 12), 0x5A5A5A5A, dtype=torch.int64, device="cuda")
    P, S, Out = d_p.data_ptr(), d_s.data_ptr(), d_o.data_ptr()

    def call(curve=0, p=P, s=S, n=n, stride=n, m=1, o=Out):
        return lib.h2_msm_points_device(curve, ctypes.c_void_p(p), ctypes.c_void_p(s), n, stride, m, ctypes.c_void_p(o), None)

    assert call() == 0
    assert call(p=0) == -1 and call(s=0) == -1 and call(o=0) == -1           # null pointers with n > 0 and m > 0
    assert call(stride=n - 1) == -1 and call(stride=n - 1, m=2) == -1          # col_stride < n
    assert call(curve=7) == -1                                                 # unknown curve
    assert call(p=P + 8) == -1 and call(s=S + 8) == -1 and call(o=Out + 8) == -1    # not 16-byte aligned
    assert call(n=(1 << 26) + 1, stride=(1 << 26) + 1) == -1                   # beyond the largest size
    torch.cuda.synchronize()
    before = d_o.cpu().numpy().copy()
    assert call(m=0) == 0 and call(m=0, p=0, s=0, o=0) == 0                   # nothing enqueued
    torch.cuda.synchronize()
    assert np.array_equal(d_o.cpu().numpy(), before)
    assert call(n=0, stride=0, m=3, p=0, s=0) == 0                             # m identities
    torch.cuda.synchronize()
    assert not d_o.cpu().numpy().any()
    out = (ctypes.c_uint64 * 12)()
    assert lib.h2_msm_points(0, None, None, 4, out) == -1
    assert lib.h2_msm_points(7, None, None, 0, out) == -1
