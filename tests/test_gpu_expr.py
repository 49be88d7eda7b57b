"""GPU: h2_expr_eval_device against big integers, over the three scalar fields.

The device output is compared byte for byte with the DAG's big-integer value on every row and with the kernel's model
(pyref.expr_kernel_row on the dumped code, with the magnitude assertions of test_expr_public.py) on a sample.  The
shapes are the smallest at which the kernel can still go wrong: fewer rows than one 64-lane block, several blocks,
several instances with their own columns and variables and a wider output stride, rotations that wrap at both ends,
periodic columns, programs shorter than the two-ahead prefetch, the live-value counts around the register / LDS and
64 KiB boundaries, a caller's stream.  The refusals enqueue nothing: a sentinel output stays as it was."""
import ctypes
import random

import numpy as np
import pytest

import test_expr_program as T
from test_expr_public import (ADD, COL, CONST, CURVE_NAMES, EINVAL, FIELDS, MUL, SUB, VAR, check_row, compile_public, dump,
                              eval_dag, info, mont_words, n_cols_of, random_dag, reductions_of, working_table)

import torch

SENTINEL = 0x5A5A5A5A5A5A5A5A


def to_device(values):
    """API integers -> a (len, 4) int64 CUDA tensor"""
    raw = b"".join(int(v).to_bytes(32, "little") for v in values)
    return torch.from_numpy(np.frombuffer(raw, dtype=np.uint64).view(np.int64).reshape(-1, 4).copy()).cuda()


def rows_of(t):
    raw = t.cpu().numpy().tobytes()
    return [int.from_bytes(raw[32 * i:32 * i + 32], "little") for i in range(len(raw) // 32)]


def random_cols(rng, p, lengths):
    """one column of random elements per length, the extremes (0, p - 1) mixed in"""
    return [[rng.choice((0, p - 1, rng.randrange(p), rng.randrange(p))) for _ in range(n)] for n in lengths]


_DOMAINS = {}


def domain_of(h2, curve):
    if curve not in _DOMAINS:
        from halo2_prover_amd.domain import EvaluationDomain
        _DOMAINS[curve] = EvaluationDomain(2, 4, CURVE_NAMES[curve])
    return _DOMAINS[curve]


class Case:
    """one compiled DAG: the public Python class, the dumped code and the field"""

    def __init__(self, h2, curve, nodes, consts, n_vars, n_cols=None):
        self.h2, self.curve, self.p = h2, curve, FIELDS[curve]
        self.nodes, self.consts, self.n_vars = nodes, consts, n_vars
        self.n_cols = n_cols_of(nodes) if n_cols is None else n_cols
        self.prog = h2.ExprProgram(nodes, consts, self.n_cols, n_vars, CURVE_NAMES[curve])
        self.code = dump(h2.load(), self.prog.handle, n_vars)
        self.reductions = reductions_of(self.code)

    def run(self, cols, variables, log_rows, step, out=None, out_stride=None):
        dev = [[to_device(c) for c in inst] for inst in cols]
        res = self.prog.eval(domain_of(self.h2, self.curve), dev, variables, log_rows, step, out=out, out_stride=out_stride)
        torch.cuda.synchronize()
        return res

    def check(self, cols, variables, log_rows, step, model_rows=24, out_stride=None):
        """cols: m lists of columns (API integers); variables: m lists of canonical ints.  Every row of every instance
        against the big-integer value, model_rows of them against the model; -> the (m, rows) results"""
        m, rows = len(cols), 1 << log_rows
        out = None
        if out_stride is not None:
            out = torch.full((m, out_stride, 4), SENTINEL, dtype=torch.int64, device="cuda")
        res = self.run(cols, variables, log_rows, step, out, out_stride)
        stride = rows if out_stride is None else out_stride
        assert tuple(res.shape) == (m, stride, 4)
        got = rows_of(res)
        picks = set(range(rows)) if rows <= model_rows else set(random.Random(rows).sample(range(rows), model_rows - 4)) | {
            0, 1, rows - 2, rows - 1}
        for q in range(m):
            cw = working_table(self.code, variables[q], self.p)
            for i in range(rows):
                def column_at(c, rot, i=i, q=q):
                    col = cols[q][c]
                    return col[(i + rot * step) & (len(col) - 1)]
                want = eval_dag(self.p, self.nodes, self.consts, variables[q], column_at) * (1 << 256) % self.p
                assert got[q * stride + i] == want, ("instance", q, "row", i)
                if i in picks:
                    assert check_row(self.p, self.code["code"], cw, column_at, self.reductions) == want
            assert all(v == SENTINEL | SENTINEL << 64 | SENTINEL << 128 | SENTINEL << 192
                       for v in got[q * stride + rows:(q + 1) * stride]), "rows past 2^log_rows were written"
        return [got[q * stride:q * stride + rows] for q in range(m)]

    def release(self):
        self.prog.release()


def some_vars(rng, p, n_vars):
    return [rng.choice((0, 1, p - 1, rng.randrange(p))) for _ in range(n_vars)]


@pytest.mark.gpu
@pytest.mark.parametrize("curve", [0, 1, 2])
def test_gpu_random_dags_16_64_and_256_rows(h2, curve):
    rng = random.Random(0x5EED + curve)
    p = FIELDS[curve]
    for n, log_rows in ((12, 4), (40, 6), (120, 8), (300, 4)):
        nodes, consts = random_dag(rng, p, n, 5, 3)
        case = Case(h2, curve, nodes, consts, 3, n_cols=5)
        case.check([random_cols(rng, p, [1 << log_rows] * 5)], [some_vars(rng, p, 3)], log_rows, 1)
        case.release()


@pytest.mark.gpu
@pytest.mark.parametrize("curve", [0, 1, 2])
def test_gpu_three_instances_with_their_own_columns_and_variables(h2, curve):
    """m = 3, out_stride > rows: the sentinel behind every instance's rows survives, and the result of the one launch is
    that of three launches with m = 1; a second evaluation of the same handle with other variables"""
    rng = random.Random(0x33 + curve)
    p = FIELDS[curve]
    nodes, consts = random_dag(rng, p, 60, 4, 2)
    k = len(nodes)                                   # root * v0 + v1: whatever the random part does, both variables count
    nodes += [(VAR, 0, 0, 0), (MUL, k - 1, k, 0), (VAR, 0, 0, 1), (ADD, k + 1, k + 2, 0)]
    case = Case(h2, curve, nodes, consts, 2, n_cols=4)
    log_rows, rows = 7, 128
    cols = [random_cols(rng, p, [rows] * 4) for _ in range(3)]
    variables = [[0, p - 1], [1, rng.randrange(p)], [rng.randrange(p), rng.randrange(p)]]
    together = case.check(cols, variables, log_rows, 2, out_stride=rows + 37)
    for q in range(3):
        alone = rows_of(case.run([cols[q]], [variables[q]], log_rows, 2))
        assert alone == together[q], q
    again = case.check(cols, variables[::-1], log_rows, 2, model_rows=8)
    assert again[0] != together[0] and again[2] != together[2]
    case.release()


@pytest.mark.gpu
@pytest.mark.parametrize("curve", [0, 1, 2])
def test_gpu_rotations_wrap_at_both_ends(h2, curve):
    rng = random.Random(0x707 + curve)
    p = FIELDS[curve]
    rots = (0, 1, -1, 127, -128, 7)
    nodes = [(COL, k % 3, 0, r) for k, r in enumerate(rots)]
    acc = 0
    for k in range(1, len(rots)):
        nodes.append((MUL if k % 2 else SUB, acc, k, 0))
        acc = len(nodes) - 1
    case = Case(h2, curve, nodes, [], 0)
    for step in (1, 2, 8):
        for log_rows in (6, 8):
            case.check([random_cols(rng, p, [1 << log_rows] * 3)], [[]], log_rows, step, model_rows=12)
    case.release()


@pytest.mark.gpu
@pytest.mark.parametrize("curve", [0, 1, 2])
def test_gpu_columns_of_length_1_4_and_full(h2, curve):
    rng = random.Random(0x71 + curve)
    p = FIELDS[curve]
    nodes = [(COL, 0, 0, 0), (COL, 1, 0, 1), (COL, 2, 0, -1), (MUL, 0, 1, 0), (ADD, 3, 2, 0), (COL, 1, 0, 3), (MUL, 4, 5, 0),
             (VAR, 0, 0, 0), (SUB, 6, 7, 0)]
    case = Case(h2, curve, nodes, [], 1)
    for log_rows, step in ((6, 1), (8, 2)):
        case.check([random_cols(rng, p, [1 << log_rows, 4, 1])], [[rng.randrange(p)]], log_rows, step)
        case.check([random_cols(rng, p, [1, 1 << log_rows, 4])], [[p - 1]], log_rows, step)
    case.release()


@pytest.mark.gpu
@pytest.mark.parametrize("curve", [0, 1, 2])
def test_gpu_programs_of_one_to_three_instructions(h2, curve):
    """shorter than the two-ahead prefetch; a leaf root is one product with one"""
    rng = random.Random(3 + curve)
    p = FIELDS[curve]
    c0, c1, c2 = (COL, 0, 0, 0), (COL, 1, 0, 1), (COL, 2, 0, -1)
    cases = {1: [c0, c1, c2, (SUB, 0, 1, 0)],
             2: [c0, c1, (MUL, 0, 1, 0), c2, (ADD, 2, 3, 0)],
             3: [c0, c1, (MUL, 0, 1, 0), c2, (SUB, 3, 2, 0), (CONST, 0, 0, 0), (MUL, 4, 5, 0)]}
    for n_instr, nodes in cases.items():
        case = Case(h2, curve, nodes, [p - 1], 0, n_cols=3)
        assert case.code["stats"][0] == n_instr
        for cols in ([[0] * 64] * 3, [[p - 1] * 64] * 3, random_cols(rng, p, [64] * 3)):
            case.check([cols], [[]], 6, 1)
        case.release()
    for nodes, n_vars in (([c0, c1], 0), ([(VAR, 0, 0, 0)], 1)):
        case = Case(h2, curve, nodes, [], n_vars, n_cols=2)
        assert case.code["stats"][:2] == (1, 1)
        case.check([random_cols(rng, p, [16, 16])], [some_vars(rng, p, n_vars)], 4, 1)
        case.release()


def live_case(h2, curve, slots):
    """the live_dag of test_expr_program.py whose program needs exactly `slots` live values"""
    lib = h2.load()
    for n in range(max(1, slots - 8), 2 * slots + 2):
        nodes = T.live_dag(n)
        rc, h = compile_public(lib, curve, nodes, [], n + 1, 0)
        assert rc == 0
        got = info(lib, h).slots
        assert lib.h2_expr_release(h) == 0
        if got == slots:
            return Case(h2, curve, nodes, [], 0)
    raise AssertionError("no live_dag needs %d slots" % slots)


@pytest.mark.gpu
@pytest.mark.parametrize("curve,slots", [(0, 4), (0, 5), (1, 4), (1, 5), (2, 4), (2, 5), (0, 33), (1, 33)])
def test_gpu_live_values_in_registers_and_lds(h2, curve, slots):
    """4 slots: registers only; 5: the first one in LDS; 33: the first count past 64 KiB of LDS"""
    rng = random.Random(slots + curve)
    case = live_case(h2, curve, slots)
    assert case.prog.info()["lds_bytes"] == max(1, slots - 4) * T.SLOT_BYTES
    case.check([random_cols(rng, FIELDS[curve], [64] * case.n_cols)], [[]], 6, 1, model_rows=6)
    case.check([[[0] * 128] * case.n_cols], [[]], 7, 1, model_rows=4)
    case.release()


@pytest.mark.gpu
def test_gpu_76_live_values_are_refused_at_compile_time(h2):
    lib = h2.load()
    for curve in (0, 1, 2):
        refused = slots = None
        for n in range(70, 90):
            rc, h = compile_public(lib, curve, T.live_dag(n), [], n + 1, 0)
            if rc != 0:
                refused = (rc, slots)
                break
            slots = info(lib, h).slots
            assert lib.h2_expr_release(h) == 0
        assert refused == (EINVAL, 75)
    case = live_case(h2, 1, 5)                      # and the device is fine afterwards
    case.check([random_cols(random.Random(1), FIELDS[1], [64] * case.n_cols)], [[]], 6, 1, model_rows=4)
    case.release()


@pytest.mark.gpu
def test_gpu_4096_rows_on_a_callers_stream(h2):
    rng = random.Random(0x57)
    curve, p = 2, FIELDS[2]
    nodes, consts = random_dag(rng, p, 30, 3, 2)
    case = Case(h2, curve, nodes, consts, 2, n_cols=3)
    cols = [random_cols(rng, p, [4096, 4096, 16])]
    variables = [some_vars(rng, p, 2)]
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        case.check(cols, variables, 12, 4, model_rows=16)
    case.release()


@pytest.mark.gpu
def test_gpu_more_instances_than_one_grid_holds(h2):
    """m = 65537 instances of one row run as two groups on the stream (grid.y holds 65535)"""
    rng = random.Random(0x10001)
    curve, p = 1, FIELDS[1]
    nodes = [(COL, 0, 0, 0), (VAR, 0, 0, 0), (MUL, 0, 1, 0), (VAR, 0, 0, 1), (SUB, 2, 3, 0)]
    case = Case(h2, curve, nodes, [], 2)
    m = 65537
    col = to_device([rng.randrange(p)])
    api = rows_of(col)[0]
    variables = [[rng.randrange(p), q] for q in range(m)]
    res = case.prog.eval(domain_of(h2, curve), [[col]] * m, variables, 0, 1)
    torch.cuda.synchronize()
    got = rows_of(res)
    x = api * pow(1 << 256, -1, p) % p
    assert got == [(x * v0 - v1) * (1 << 256) % p for v0, v1 in variables]
    case.release()


# ---- the refusals of h2_expr_eval_device: nothing is enqueued --------------------------------------------------------------
def raw_eval(lib, handle, ptrs, log_len, var_words, m, log_rows, step, out_ptr, out_stride):
    pa = (ctypes.c_void_p * max(1, len(ptrs)))(*ptrs)
    ll = (ctypes.c_uint32 * max(1, len(log_len)))(*log_len)
    return lib.h2_expr_eval_device(handle, pa, ll, var_words, m, log_rows, step, ctypes.c_void_p(out_ptr), out_stride, None)


@pytest.mark.gpu
@pytest.mark.parametrize("curve", [0, 1, 2])
def test_gpu_eval_refuses_before_anything_is_enqueued(h2, curve):
    lib = h2.load()
    p = FIELDS[curve]
    rng = random.Random(0xBAD + curve)
    nodes = [(COL, 0, 0, 0), (COL, 1, 0, 1), (MUL, 0, 1, 0), (VAR, 0, 0, 0), (ADD, 2, 3, 0)]
    rc, h = compile_public(lib, curve, nodes, [], 2, 1)
    assert rc == 0
    rows, log_rows = 64, 6
    cols = random_cols(rng, p, [rows, rows])
    buf = torch.cat([to_device(cols[0]), to_device(cols[1]), torch.full((2 * rows, 4), SENTINEL, dtype=torch.int64, device="cuda")])
    base = buf.data_ptr()
    c0, c1, out = base, base + 32 * rows, base + 64 * rows
    good = mont_words([5], p)
    torch.cuda.synchronize()
    before = buf.clone()
    bad = {
        "d_out overlaps column 1": ([c0, c1], [6, 6], good, 1, log_rows, c1 + 32 * (rows - 1), rows),
        "d_out is a column": ([c0, c1], [6, 6], good, 1, log_rows, c0, rows),
        "the second instance's rows overlap": ([c0, out + 32 * rows, c0, c1], [6, 6], mont_words([5, 5], p), 2, log_rows, out, rows),
        "log_len > log_rows": ([c0, c1], [6, 7], good, 1, log_rows, out, rows),
        "log_rows > 28": ([c0, c1], [6, 6], good, 1, 29, out, 1 << 29),
        "out_stride < rows": ([c0, c1], [6, 6], good, 1, log_rows, out, rows - 1),
        "misaligned column": ([c0, c1 + 8], [6, 5], good, 1, log_rows, out, rows),
        "misaligned d_out": ([c0, c1], [6, 6], good, 1, log_rows, out + 8, rows),
        "null column": ([c0, 0], [6, 6], good, 1, log_rows, out, rows),
        "null d_out": ([c0, c1], [6, 6], good, 1, log_rows, 0, rows),
        "variable = p": ([c0, c1], [6, 6], mont_words([p], p), 1, log_rows, out, rows),
        "variable = 2^256 - 1": ([c0, c1], [6, 6], mont_words([(1 << 256) - 1], p), 1, log_rows, out, rows),
    }
    for name, (ptrs, log_len, var_words, m, lr, out_ptr, stride) in bad.items():
        assert raw_eval(lib, h, ptrs, log_len, var_words, m, lr, 1, out_ptr, stride) == EINVAL, name
    assert lib.h2_expr_eval_device(h, None, None, good, 1, log_rows, 1, ctypes.c_void_p(out), rows, None) == EINVAL
    assert raw_eval(lib, h, [c0, c1], [6, 6], None, 1, log_rows, 1, out, rows) == EINVAL
    assert raw_eval(lib, h + 1000, [c0, c1], [6, 6], good, 1, log_rows, 1, out, rows) == -4
    assert raw_eval(lib, h, [c0, c1], [6, 6], good, 0, log_rows, 1, out, rows) == 0          # m = 0: nothing to do
    torch.cuda.synchronize()
    assert torch.equal(buf, before)
    # and the same arguments put right do run
    assert raw_eval(lib, h, [c0, c1], [6, 6], good, 1, log_rows, 1, out, rows) == 0
    torch.cuda.synchronize()
    got = rows_of(buf[2 * rows:3 * rows])
    for i in range(rows):
        want = eval_dag(p, nodes, [], [5], lambda c, rot, i=i: cols[c][(i + rot) % rows]) * (1 << 256) % p
        assert got[i] == want
    assert torch.equal(buf[3 * rows:], before[3 * rows:])
    # a column inside the unwritten rows between two instances overlaps nothing that is written; one row further it
    # would reach the second instance's first row
    wide = torch.full((3 * rows, 4), SENTINEL, dtype=torch.int64, device="cuda")
    wide[rows:2 * rows] = to_device(cols[1])
    w = wide.data_ptr()
    gap = w + 32 * rows
    two = mont_words([5, 7], p)
    torch.cuda.synchronize()
    assert raw_eval(lib, h, [c0, gap + 32, c0, gap + 32], [6, 6], two, 2, log_rows, 1, w, 2 * rows) == EINVAL
    assert raw_eval(lib, h, [c0, gap - 32, c0, gap - 32], [6, 6], two, 2, log_rows, 1, w, 2 * rows) == EINVAL
    assert raw_eval(lib, h, [c0, gap, c0, gap], [6, 6], two, 2, log_rows, 1, w, 2 * rows) == 0
    torch.cuda.synchronize()
    got = rows_of(wide)
    assert got[rows:2 * rows] == cols[1]
    for q, v in enumerate((5, 7)):
        for i in range(rows):
            want = eval_dag(p, nodes, [], [v], lambda c, rot, i=i: cols[c][(i + rot) % rows]) * (1 << 256) % p
            assert got[2 * rows * q + i] == want
    assert lib.h2_expr_release(h) == 0
    assert raw_eval(lib, h, [c0, c1], [6, 6], good, 1, log_rows, 1, out, rows) == -4
