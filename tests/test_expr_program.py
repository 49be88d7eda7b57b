"""The quotient program (h2_prover.hip ExprProgram::compile, h2_prover_kernels.hpp expr_kernel) against big integers,
all over bn256::Fr.  A caller's expression DAG goes through the prover's own compiler (h2_selftest_host what = 7) and,
on the GPU, through the launch create_proof makes (h2_selftest_expr_run).

* CPU: pyref.expr_kernel_row runs the compiled code over concrete rows with the kernel's exact limbs (column operands
  (api << 5) - 16 p, constants unpacked from c 2^261 mod p, sums through fe29_norm, products through the exact
  fe29_mul model, the result through fe29_to_api).  On random DAGs, adversarial ones and the three circuits' own
  programs (what = 6), with columns at the extremes (API integer 0 = the operand -16 p, p - 1, and the two
  alternating): every product operand meets fe29_mul's limb bounds, every value kept or forwarded is at most 32 p and a
  sum before its reduction at most 64 p, the root below 64 p, and the output equals the DAG's big-integer value (for
  the circuits' programs, whose DAG is not exported: the code's own value mod p).  Malformed DAGs are refused.
* GPU: the device's output equals the model's and the big-integer value byte for byte: random DAGs, sum / difference
  and product chains, programs of 1-3 instructions, rotations and steps that wrap at both ends, short periodic
  columns, 16 to 2^18 rows, and the live-value counts around the LDS: 4 and 5 slots, the first above 64 KiB, the last
  that fits and one past it (H2_EINVAL, nothing launched)."""
import ctypes
import random
import struct

import numpy as np
import pytest

import pyref as R

P = R.BN_FR.p
INV256 = pow(1 << 256, -1, P)
EINVAL = -1
CONST, COL, ADD, SUB, MUL = 0, 1, 2, 3, 4
SLOT_BYTES = 9 * 64 * 4                 # LDS per slot beyond the four register slots: nine limbs of 64 rows
LDS_MAX = 160 * 1024


@pytest.fixture(scope="module")
def lib():
    import halo2_prover_amd
    return halo2_prover_amd.load()


# ---- DAGs ------------------------------------------------------------------------------------------------------------
def dag_bytes(nodes, consts):
    blob = struct.pack("<2I", len(nodes), len(consts))
    blob += b"".join(struct.pack("<4i", *nd) for nd in nodes)
    return blob + b"".join(int(c).to_bytes(32, "little") for c in consts)


def compile_dag(lib, nodes, consts):
    """-> (status, program) with program = dict(stats, code, table) as what = 7 reports it"""
    blob = dag_bytes(nodes, consts)
    cap = 24 + 24 * len(nodes) + 32 * (len(consts) + 1) + 64
    out = ctypes.create_string_buffer(cap)
    n = ctypes.c_size_t(0)
    rc = lib.h2_selftest_host(7, blob, len(blob), out, cap, ctypes.byref(n))
    if rc != 0:
        return rc, None
    return rc, parse_report(out.raw[:n.value], with_table=True)


def parse_report(raw, with_table):
    stats = struct.unpack("<6I", raw[:24])
    n_instr, n_consts = stats[0], stats[4]
    code = [struct.unpack("<3I", raw[24 + 12 * i:36 + 12 * i]) for i in range(n_instr)]
    end = 24 + 12 * n_instr
    table = None
    if with_table:
        assert len(raw) == end + 32 * n_consts
        table = [int.from_bytes(raw[end + 32 * k:end + 32 * k + 32], "little") for k in range(n_consts)]
        assert all(0 <= c < P for c in table)
    else:
        assert len(raw) == end
    return {"stats": stats, "code": code, "table": table}


def circuit_program(lib, circuit):
    out = ctypes.create_string_buffer(1 << 20)
    n = ctypes.c_size_t(0)
    assert lib.h2_selftest_host(6, bytes([circuit]), 1, out, 1 << 20, ctypes.byref(n)) == 0
    return parse_report(out.raw[:n.value], with_table=False)


def eval_dag(nodes, consts, column_at):
    """the root's value x (mod p); column_at(c, rot) -> the API integer x 2^256 the row reads"""
    v = []
    for op, a, b, x in nodes:
        if op == CONST:
            v.append(consts[x] % P)
        elif op == COL:
            v.append(column_at(a, x) * INV256 % P)
        elif op == ADD:
            v.append((v[a] + v[b]) % P)
        elif op == SUB:
            v.append((v[a] - v[b]) % P)
        else:
            v.append(v[a] * v[b] % P)
    return v[-1]


def eval_code(code, consts_working, column_at):
    """the compiled code's own value mod p, in the working form x 2^261 (no lazy magnitudes): the API integer"""
    rp_inv = pow(R.FE29_R, -1, P)
    slots, r = {}, 0
    for op_dst, aw, bw in code:
        def operand(w):
            kind, low = w >> 30, w & 0x3FFFFFFF
            if kind == R.X_SLOT:
                return slots.get(low, 0)
            if kind == R.X_PREV:
                return r
            if kind == R.X_CONST:
                return consts_working[low]
            return column_at(low >> 8, (low & 0xFF) - 128) * 32 % P
        a, b = operand(aw), operand(bw)
        op, dst = op_dst >> 24, op_dst & 0xFFFFFF
        r = a * b * rp_inv % P if op == 2 else (a + b) % P if op == 0 else (a - b) % P
        if dst != R.X_NO_STORE:
            slots[dst] = r
    return r * rp_inv * (1 << 256) % P


def working(table):
    return [c * R.FE29_R % P for c in table]


def check_row(code, consts_working, column_at, one_idx=None):
    """model one row, assert the magnitudes the kernel relies on; -> the API integer of the result"""
    steps = []
    out = R.expr_kernel_row(code, consts_working, column_at, P, steps)
    last = len(code) - 1
    for t, (op, a, b, r, dst) in enumerate(steps):
        if op == 2:
            assert R.fe29_mul_limbs_ok(a, b), ("product operand past the limb bounds", t)
        v = abs(R.fe29_value(r))
        nxt = code[t + 1] if t < last else None
        reduced = (op != 2 and dst == R.X_NO_STORE and nxt is not None and nxt[0] >> 24 == 2 and
                   nxt[1] >> 30 == R.X_PREV and nxt[2] >> 30 == R.X_CONST and
                   (one_idx is None or nxt[2] & 0x3FFFFFFF == one_idx))
        if t == last:
            assert v < 64 * P, ("root", t, v / P)
        elif reduced:
            assert v <= 64 * P, ("sum before its reduction", t, v / P)
        else:
            assert v <= 32 * P, ("value kept or forwarded", t, v / P)
    assert 0 <= out < P
    return out


def patterns(rng):
    """column_at factories: the extremes (API integer 0 -> operand -16 p, p - 1, the two alternating) and random"""
    rnd = {}

    def random_at(c, rot):
        return rnd.setdefault((c, rot), rng.randrange(P))
    return {"zero": lambda c, rot: 0, "max": lambda c, rot: P - 1,
            "alt0": lambda c, rot: 0 if (c + rot) % 2 == 0 else P - 1,
            "alt1": lambda c, rot: P - 1 if (c + rot) % 2 == 0 else 0, "random": random_at}


def check_dag(lib, nodes, consts, rng):
    rc, prog = compile_dag(lib, nodes, consts)
    assert rc == 0
    one_idx = prog["table"].index(1)
    cw = working(prog["table"])
    for name, column_at in patterns(rng).items():
        got = check_row(prog["code"], cw, column_at, one_idx)
        assert got == eval_dag(nodes, consts, column_at) * (1 << 256) % P, name
    return prog


def random_dag(rng, n, ncols, nconsts=4, rots=(0, 1, -1, 7, -7)):
    """n nodes: a quarter leaves (columns at rotations, constants), the rest add / sub / mul of earlier nodes, mostly
    recent ones (depth) and some anywhere (shared subexpressions)"""
    consts = [rng.choice((0, 1, P - 1, rng.randrange(P))) for _ in range(nconsts)]
    nodes = []
    for _ in range(max(2, n // 4)):
        if rng.random() < 0.75:
            nodes.append((COL, rng.randrange(ncols), 0, rng.choice(rots)))
        else:
            nodes.append((CONST, 0, 0, rng.randrange(nconsts)))
    while len(nodes) < n:
        k = len(nodes)
        a = rng.randrange(max(0, k - 4), k) if rng.random() < 0.7 else rng.randrange(k)
        b = rng.randrange(k)
        nodes.append((rng.choice((ADD, SUB, MUL, MUL)), a, b, 0))
    return nodes, consts


def chain(op, ncols, start=0, rot=0):
    nodes = [(COL, start + c, 0, rot) for c in range(ncols)]
    acc = 0
    for c in range(1, ncols):
        nodes.append((op(c) if callable(op) else op, acc, c, 0))
        acc = len(nodes) - 1
    return nodes


def live_dag(n):
    """v_j = col_j col_{j+1} (j < n), then (sum v_j) (prod v_j): all n products live at once"""
    nodes = [(COL, c, 0, 0) for c in range(n + 1)]
    v = []
    for j in range(n):
        nodes.append((MUL, j, j + 1, 0))
        v.append(len(nodes) - 1)
    s = v[0]
    for j in v[1:]:
        nodes.append((ADD, s, j, 0))
        s = len(nodes) - 1
    pr = v[0]
    for j in v[1:]:
        nodes.append((MUL, pr, j, 0))
        pr = len(nodes) - 1
    nodes.append((MUL, s, pr, 0))
    return nodes


def live_dag_for(lib, slots):
    """the live_dag whose program needs exactly `slots` slots"""
    for n in range(1, 2 * slots + 2):
        rc, prog = compile_dag(lib, live_dag(n), [])
        assert rc == 0
        if prog["stats"][3] == slots:
            return live_dag(n), prog
    raise AssertionError("no live_dag needs %d slots" % slots)


def adversarial_dags():
    """(name, nodes, consts, reductions expected): long sums and differences of columns, balanced sum trees, products
    of the largest sums, sums of products, constants p - 1"""
    out = []
    out.append(("sum40", chain(ADD, 40), [], True))
    out.append(("diff40", chain(SUB, 40), [], True))
    out.append(("alt64", chain(lambda c: ADD if c % 3 else SUB, 64), [], True))
    # ((c0 + c1) + (c2 + c3)) + ...: balanced, every level doubles the bound
    nodes = [(COL, c, 0, 0) for c in range(32)]
    level = list(range(32))
    while len(level) > 1:
        nxt = []
        for i in range(0, len(level), 2):
            nodes.append((ADD if i % 4 == 0 else SUB, level[i], level[i + 1], 0))
            nxt.append(len(nodes) - 1)
        level = nxt
    out.append(("tree32", nodes, [], True))
    # (sum of 20 columns) * (difference chain of 20 columns), then squared
    nodes = chain(ADD, 20)
    s = len(nodes) - 1
    more = chain(SUB, 20, start=20)
    off = len(nodes)
    nodes += [(op, a + off if op != COL else a, b + off if op != COL else b, x) for op, a, b, x in more]
    d = len(nodes) - 1
    nodes.append((MUL, s, d, 0))
    nodes.append((MUL, len(nodes) - 1, len(nodes) - 1, 0))
    out.append(("sumxdiff", nodes, [], True))
    # sum of 48 products of columns, then minus a sum of constants p - 1
    nodes = [(COL, c, 0, 0) for c in range(49)]
    prods = []
    for c in range(48):
        nodes.append((MUL, c, c + 1, 0))
        prods.append(len(nodes) - 1)
    acc = prods[0]
    for j in prods[1:]:
        nodes.append((ADD, acc, j, 0))
        acc = len(nodes) - 1
    nodes.append((CONST, 0, 0, 0))
    k = len(nodes) - 1
    for _ in range(40):
        nodes.append((SUB, acc, k, 0))
        acc = len(nodes) - 1
    nodes.append((MUL, acc, acc, 0))
    out.append(("sumprod", nodes, [P - 1], True))
    # x = c0 + c1 + ... (31 terms, just below the bound before a reduction), x * x, x * c
    nodes = chain(ADD, 31)
    x = len(nodes) - 1
    nodes.append((MUL, x, x, 0))
    nodes.append((MUL, len(nodes) - 1, 0, 0))
    out.append(("square_of_sum", nodes, [], True))
    return out


# ---- CPU ---------------------------------------------------------------------------------------------------------------
def test_random_dags_model_matches_big_integers_within_bounds(lib):
    rng = random.Random(0xE7)
    for n in (5, 6, 9, 17, 33, 64, 120, 200, 300):
        for _ in range(2):
            nodes, consts = random_dag(rng, n, ncols=6)
            check_dag(lib, nodes, consts, rng)


def test_adversarial_dags_stay_within_the_bounds(lib):
    rng = random.Random(0xAD)
    for name, nodes, consts, reduces in adversarial_dags():
        prog = check_dag(lib, nodes, consts, rng)
        if reduces:
            assert prog["stats"][5] > 0, name


@pytest.mark.parametrize("circuit", [0, 1, 2])
def test_circuit_programs_stay_within_the_bounds(lib, circuit):
    """the prover's own programs (constants unknown here: every one at the largest working value p - 1, then random);
    the model's result equals the code's value mod p"""
    prog = circuit_program(lib, circuit)
    rng = random.Random(circuit)
    n_consts = prog["stats"][4]
    for cw in ([P - 1] * n_consts, [rng.randrange(P) for _ in range(n_consts)]):
        for name, column_at in patterns(rng).items():
            assert check_row(prog["code"], cw, column_at) == eval_code(prog["code"], cw, column_at), (circuit, name)


def test_what7_reports_the_program_and_its_constants(lib):
    nodes = chain(ADD, 3)
    rc, prog = compile_dag(lib, nodes, [])
    assert rc == 0
    n_instr, n_mul, n_col, n_slots, n_consts, n_reduce = prog["stats"]
    # (c0 + c1) + c2: 16 p + 16 p is kept, 48 p is reduced by a product with the one constant compile adds
    assert (n_instr, n_mul, n_col, n_consts, n_reduce) == (3, 1, 3, 1, 1)
    assert prog["code"][2] == ((2 << 24) | R.X_NO_STORE, R.X_PREV << 30, R.X_CONST << 30)
    assert prog["table"] == [1]


def test_malformed_dags_are_refused(lib):
    col = (COL, 0, 0, 0)
    bad = {
        "later node": [col, (COL, 1, 0, 0), (ADD, 0, 3, 0), (ADD, 0, 2, 0)],
        "itself": [col, (ADD, 0, 1, 0)],
        "negative node": [col, (MUL, -1, 0, 0)],
        "rotation 128": [(COL, 0, 0, 128), col, (ADD, 0, 1, 0)],
        "rotation -129": [(COL, 0, 0, -129), col, (ADD, 0, 1, 0)],
        "rotation 200": [(COL, 0, 0, 200), col, (ADD, 0, 1, 0)],
        "column 2^22": [(COL, 1 << 22, 0, 0), col, (ADD, 0, 1, 0)],
        "negative column": [(COL, -1, 0, 0), col, (ADD, 0, 1, 0)],
        "root constant": [col, (CONST, 0, 0, 0)],
        "root column": [(CONST, 0, 0, 0), col],
        "unknown op": [col, (COL, 1, 0, 0), (5, 0, 1, 0)],
        "no such constant": [col, (CONST, 0, 0, 1), (ADD, 0, 1, 0)],
    }
    for name, nodes in bad.items():
        assert compile_dag(lib, nodes, [7])[0] == EINVAL, name
        assert run_device(lib, nodes, [7], [[1] * 64] * 2, 6, 1)[0] == EINVAL, name
    # the edges that are fine: rotations -128 and 127, column 2^22 - 1
    assert compile_dag(lib, [(COL, (1 << 22) - 1, 0, -128), (COL, 0, 0, 127), (MUL, 0, 1, 0)], [])[0] == 0
    ok = [col, (COL, 1, 0, 0), (ADD, 0, 1, 0)]
    assert compile_dag(lib, ok, [P])[0] == EINVAL                     # constant not canonical
    blob = dag_bytes(ok, [])
    n = ctypes.c_size_t(0)
    out = ctypes.create_string_buffer(256)
    assert lib.h2_selftest_host(7, blob[:-1], len(blob) - 1, out, 256, ctypes.byref(n)) == EINVAL
    assert run_device(lib, ok, [], [[P] * 64, [1] * 64], 6, 1)[0] == EINVAL         # column element not canonical
    assert run_device(lib, ok, [], [[1] * 64], 6, 1)[0] == EINVAL                    # column 1 does not exist


def test_live_values_and_the_lds_limit(lib):
    """slots 0-3 are registers, each further one SLOT_BYTES of LDS: 33 slots is the first count past 64 KiB, 75 the
    last that fits 160 KiB; 76 is refused by the device hook before any device is looked at"""
    lds = {s: max(1, s - 4) * SLOT_BYTES for s in (4, 5, 32, 33, 75, 76)}
    assert lds[32] <= 64 * 1024 < lds[33] and lds[75] <= LDS_MAX < lds[76]
    for slots in (4, 5, 33, 75, 76):
        nodes, prog = live_dag_for(lib, slots)
        if slots <= 5:
            check_dag(lib, nodes, [], random.Random(slots))
    nodes, _ = live_dag_for(lib, 76)
    cols = [[1] * 64 for _ in range(max(nd[1] for nd in nodes if nd[0] == COL) + 1)]
    assert run_device(lib, nodes, [], cols, 6, 1)[0] == EINVAL


# ---- GPU ---------------------------------------------------------------------------------------------------------------
def run_device(lib, nodes, consts, cols, log_en, step, sentinel=False):
    """-> (status, results as API integers, the six counters)"""
    blob = dag_bytes(nodes, consts)
    log_len = np.array([len(c).bit_length() - 1 for c in cols], dtype=np.uint32)
    assert all(len(c) == 1 << int(k) for c, k in zip(cols, log_len))
    flat = np.frombuffer(b"".join(int(v).to_bytes(32, "little") for c in cols for v in c), dtype=np.uint64).copy()
    en = 1 << log_en
    out = np.full(4 * en, 0xA5A5A5A5A5A5A5A5 if sentinel else 0, dtype=np.uint64)
    stats = np.zeros(6, dtype=np.uint32)
    rc = lib.h2_selftest_expr_run(blob, len(blob), flat.ctypes.data_as(ctypes.c_void_p),
                                  log_len.ctypes.data_as(ctypes.c_void_p), len(cols), log_en, step,
                                  out.ctypes.data_as(ctypes.c_void_p), stats.ctypes.data_as(ctypes.c_void_p))
    raw = out.tobytes()
    res = [int.from_bytes(raw[32 * i:32 * i + 32], "little") for i in range(en)]
    return rc, res, tuple(int(s) for s in stats), out


def random_cols(rng, ncols, length):
    """columns of random elements with the extremes (0, p - 1) mixed in"""
    return [[rng.choice((0, P - 1, rng.randrange(P), rng.randrange(P))) for _ in range(length)] for _ in range(ncols)]


def check_device(lib, nodes, consts, cols, log_en, step, model_rows=96):
    """the device's results against the big-integer value on every row and the model on up to model_rows rows"""
    rc, got, stats, _ = run_device(lib, nodes, consts, cols, log_en, step)
    assert rc == 0
    rc, prog = compile_dag(lib, nodes, consts)
    assert rc == 0 and stats == prog["stats"]
    en = 1 << log_en
    cw = working(prog["table"])
    one_idx = prog["table"].index(1)
    ends = min(16, model_rows // 4)
    picks = set(range(en)) if en <= model_rows else set(range(ends)) | set(range(en - ends, en)) | set(
        random.Random(en).sample(range(en), model_rows - 2 * ends))
    for i in range(en):
        def column_at(c, rot, i=i):
            return cols[c][(i + rot * step) & (len(cols[c]) - 1)]
        want = eval_dag(nodes, consts, column_at) * (1 << 256) % P
        assert got[i] == want, ("row", i)
        if i in picks:
            assert check_row(prog["code"], cw, column_at, one_idx) == got[i], ("row", i)
    return prog


@pytest.mark.gpu
def test_gpu_random_dags(h2):
    lib = h2.load()
    rng = random.Random(0x5EED)
    for k, n in enumerate((5, 7, 12, 20, 33, 50, 80, 130, 200, 300)):
        nodes, consts = random_dag(rng, n, ncols=6)
        log_en = (6, 8, 12)[k % 3]
        check_device(lib, nodes, consts, random_cols(rng, 6, 1 << log_en), log_en, 1)


@pytest.mark.gpu
def test_gpu_sum_difference_and_product_chains(h2):
    lib = h2.load()
    rng = random.Random(0xC4A1)
    for name, nodes, consts, reduces in adversarial_dags():
        ncols = max(nd[1] for nd in nodes if nd[0] == COL) + 1
        for cols in ([[0] * 64] * ncols, [[P - 1] * 64] * ncols, random_cols(rng, ncols, 64)):
            prog = check_device(lib, nodes, consts, cols, 6, 1)
            assert prog["stats"][5] > 0, name
    for length in (40, 64):                                       # long product chains, squares of squares
        nodes = chain(MUL, length)
        check_device(lib, nodes, [], random_cols(rng, length, 64), 6, 1)
        nodes = [(COL, 0, 0, 0)] + [(MUL, j, j, 0) for j in range(length)]
        check_device(lib, nodes, [], random_cols(rng, 1, 64), 6, 1)


@pytest.mark.gpu
def test_gpu_programs_of_one_to_three_instructions(h2):
    lib = h2.load()
    rng = random.Random(3)
    c0, c1, c2 = (COL, 0, 0, 0), (COL, 1, 0, 1), (COL, 2, 0, -1)
    cases = {1: [c0, c1, (SUB, 0, 1, 0)],
             2: [c0, c1, (MUL, 0, 1, 0), c2, (ADD, 2, 3, 0)],
             3: [c0, c1, (MUL, 0, 1, 0), c2, (SUB, 3, 2, 0), (CONST, 0, 0, 0), (MUL, 4, 5, 0)]}
    for n_instr, nodes in cases.items():
        for cols in ([[0] * 64] * 3, [[P - 1] * 64] * 3, random_cols(rng, 3, 64)):
            prog = check_device(lib, nodes, [P - 1], cols, 6, 1)
            assert prog["stats"][0] == n_instr


@pytest.mark.gpu
def test_gpu_rotations_and_steps_wrap_at_both_ends(h2):
    lib = h2.load()
    rng = random.Random(0x707)
    rots = (0, 1, -1, 7, -7, 127, -128)
    nodes = [(COL, k % 3, 0, r) for k, r in enumerate(rots)]
    acc = 0
    for k in range(1, len(rots)):
        nodes.append((MUL if k % 2 else SUB, acc, k, 0))
        acc = len(nodes) - 1
    for step in (1, 2, 8):
        for log_en in (6, 8):
            check_device(lib, nodes, [], random_cols(rng, 3, 1 << log_en), log_en, step)


@pytest.mark.gpu
def test_gpu_columns_shorter_than_the_domain(h2):
    lib = h2.load()
    rng = random.Random(0x71)
    nodes = [(COL, 0, 0, 0), (COL, 1, 0, 1), (COL, 2, 0, -1), (MUL, 0, 1, 0), (ADD, 3, 2, 0), (COL, 0, 0, 3),
             (MUL, 4, 5, 0)]
    for log_en in (6, 12):
        cols = [random_cols(rng, 1, 1 << log_en)[0], random_cols(rng, 1, 4)[0], random_cols(rng, 1, 1)[0]]
        check_device(lib, nodes, [], cols, log_en, 1)
        cols = [random_cols(rng, 1, 8)[0], random_cols(rng, 1, 1 << log_en)[0], random_cols(rng, 1, 2)[0]]
        check_device(lib, nodes, [], cols, log_en, 2)


@pytest.mark.gpu
def test_gpu_domain_sizes(h2):
    """16 rows (fewer than one 64-lane block), 64, 4096 and 2^18 with step 4"""
    lib = h2.load()
    rng = random.Random(0xD0)
    nodes, consts = random_dag(rng, 24, ncols=4)
    for log_en in (4, 6, 12):
        check_device(lib, nodes, consts, random_cols(rng, 4, 1 << log_en), log_en, 1)
    nodes = [(COL, 0, 0, 0), (COL, 1, 0, 1), (MUL, 0, 1, 0), (COL, 2, 0, -1), (SUB, 2, 3, 0), (COL, 0, 0, 2),
             (MUL, 4, 5, 0), (CONST, 0, 0, 0), (ADD, 6, 7, 0)]
    check_device(lib, nodes, [P - 1], random_cols(rng, 3, 1 << 18), 18, 4, model_rows=64)


@pytest.mark.gpu
def test_gpu_live_values_in_registers_and_lds(h2):
    """4 slots (registers only), 5 (the first LDS slot), 33 (the first count past 64 KiB of LDS), 75 (the limit) run
    and match; 76 returns H2_EINVAL and writes nothing"""
    lib = h2.load()
    rng = random.Random(0x75)
    for slots in (4, 5, 33, 75):
        nodes, prog = live_dag_for(lib, slots)
        ncols = max(nd[1] for nd in nodes if nd[0] == COL) + 1
        check_device(lib, nodes, [], random_cols(rng, ncols, 64), 6, 1, model_rows=8)
        check_device(lib, nodes, [], [[0] * 256] * ncols, 8, 1, model_rows=4)
    nodes, _ = live_dag_for(lib, 76)
    ncols = max(nd[1] for nd in nodes if nd[0] == COL) + 1
    rc, _, stats, out = run_device(lib, nodes, [], random_cols(rng, ncols, 64), 6, 1, sentinel=True)
    assert rc == EINVAL
    assert np.all(out == 0xA5A5A5A5A5A5A5A5) and not any(stats)
    nodes, _ = live_dag_for(lib, 5)                 # and the device is fine afterwards
    check_device(lib, nodes, [], random_cols(rng, 5, 64), 6, 1)
