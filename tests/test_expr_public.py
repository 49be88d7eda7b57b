"""CPU (no GPU): h2_expr_compile's programs against big integers, for each of the three scalar fields.

A DAG goes through the public compiler (h2_expr_compile), comes back through h2_expr_dump and is run row by row through
pyref.expr_kernel_row -- the kernel's exact limbs -- with that field's p.  On every row: every product operand meets
fe29_mul's limb bounds, a value kept or forwarded is at most 32 p, a sum before its reduction at most 64 p, the root below
64 p, and the output is the DAG's big-integer value.  Random DAGs of 5 to 300 nodes with variables, the sum, difference
and product chains test_expr_program.py calls adversarial, leaf roots; columns all 0, all p - 1, the two alternating and
random; variables at 0, 1 and p - 1.  For the Pasta primes p / 2^261 exceeds 1/128, so this is also the check of the
compiler's bounds there that needs no GPU (h2_expr_kernel.hpp carries the argument).  For bn256::Fr the public compiler
emits what the prover's own (h2_selftest_host what = 7) emits for the same DAG."""
import ctypes
import random
import struct

import pytest

import pyref as R
import test_expr_program as T

CONST, COL, ADD, SUB, MUL, VAR = 0, 1, 2, 3, 4, 5
FIELDS = {0: R.R_BN, 1: R.Q_PASTA, 2: R.P_PASTA}            # the scalar field of bn254, pallas, vesta
CURVE_NAMES = {0: "bn254", 1: "pallas", 2: "vesta"}
EINVAL, EHANDLE = -1, -4


@pytest.fixture(scope="module")
def lib():
    import halo2_prover_amd
    return halo2_prover_amd.load()


def mont_words(values, p):
    """canonical ints -> their Montgomery limbs (the API form) as a ctypes array of 4 u64 each"""
    arr = (ctypes.c_uint64 * max(1, 4 * len(values)))()
    for j, v in enumerate(values):
        x = v * (1 << 256) % p if 0 <= v < p else v              # a value outside the field goes through as it is
        for w in range(4):
            arr[4 * j + w] = (x >> (64 * w)) & 0xFFFFFFFFFFFFFFFF
    return arr


def compile_public(lib, curve, nodes, consts, n_cols, n_vars):
    """-> (status, handle); consts are canonical ints"""
    raw = b"".join(struct.pack("<4i", *nd) for nd in nodes)
    h = ctypes.c_uint64(0)
    rc = lib.h2_expr_compile(curve, raw, len(nodes), mont_words(consts, FIELDS[curve]), len(consts), n_cols, n_vars,
                             ctypes.byref(h))
    return rc, h.value


def dump(lib, handle, n_vars):
    n = ctypes.c_size_t(0)
    assert lib.h2_expr_dump(handle, None, 0, ctypes.byref(n)) == EINVAL and n.value >= 24 + 12 + 32
    buf = ctypes.create_string_buffer(n.value)
    assert lib.h2_expr_dump(handle, buf, n.value, ctypes.byref(n)) == 0
    raw = buf.raw[:n.value]
    stats = struct.unpack("<6I", raw[:24])
    n_instr, n_consts = stats[0], stats[4]
    code = [struct.unpack("<3I", raw[24 + 12 * i:36 + 12 * i]) for i in range(n_instr)]
    end = 24 + 12 * n_instr
    table = [int.from_bytes(raw[end + 32 * k:end + 32 * k + 32], "little") for k in range(n_consts)]
    end += 32 * n_consts
    assert len(raw) == end + 4 * n_vars
    var_slot = list(struct.unpack("<%dI" % n_vars, raw[end:]))
    return {"stats": stats, "code": code, "table": table, "var_slot": var_slot}


def info(lib, handle):
    import halo2_prover_amd.lib as L
    out = L.ExprInfo()
    assert lib.h2_expr_info(handle, ctypes.byref(out)) == 0
    return out


def eval_dag(p, nodes, consts, variables, column_at):
    """the root's value (mod p); column_at(c, rot) -> the API integer x 2^256 the row reads"""
    inv256 = pow(1 << 256, -1, p)
    v = []
    for op, a, b, x in nodes:
        if op == CONST:
            v.append(consts[x] % p)
        elif op == VAR:
            v.append(variables[x] % p)
        elif op == COL:
            v.append(column_at(a, x) * inv256 % p)
        elif op == ADD:
            v.append((v[a] + v[b]) % p)
        elif op == SUB:
            v.append((v[a] - v[b]) % p)
        else:
            v.append(v[a] * v[b] % p)
    return v[-1]


def working_table(prog, variables, p):
    """the constant table as the kernel gets it: c 2^261 mod p, the variables in their slots"""
    table = list(prog["table"])
    for v, slot in enumerate(prog["var_slot"]):
        assert table[slot] == 0
        table[slot] = variables[v]
    return [c * R.FE29_R % p for c in table]


def reductions_of(prog):
    """the instructions whose result is a sum before its reduction: an add or sub that is not stored, followed by the
    product of it with the constant one.  The compiler reports how many reductions it inserted, and the count of this
    pattern must equal it: a DAG that multiplies a sum by the constant 1 itself would be indistinguishable in the code,
    so the DAGs of these tests hold no constant 1 (a leaf root's product with one has no sum in front of it)."""
    code, one_idx = prog["code"], prog["table"].index(1)
    found = set()
    for t in range(len(code) - 1):
        ins, nxt = code[t], code[t + 1]
        if (ins[0] >> 24 != 2 and ins[0] & 0xFFFFFF == R.X_NO_STORE and nxt[0] >> 24 == 2 and nxt[1] >> 30 == R.X_PREV and
                nxt[2] >> 30 == R.X_CONST and nxt[2] & 0x3FFFFFFF == one_idx):
            found.add(t)
    assert len(found) == prog["stats"][5], "the pattern is not exactly the compiler's reductions"
    return found


def check_row(p, code, consts_working, column_at, reductions):
    """model one row and assert the magnitudes the kernel relies on (reductions: reductions_of the program); -> the API
    integer of the result"""
    steps = []
    out = R.expr_kernel_row(code, consts_working, column_at, p, steps)
    last = len(code) - 1
    for t, (op, a, b, r, dst) in enumerate(steps):
        if op == 2:
            assert R.fe29_mul_limbs_ok(a, b), ("product operand past the limb bounds", t)
        v = abs(R.fe29_value(r))
        if t == last:
            assert v < 64 * p, ("root", t, v / p)
        elif t in reductions:
            assert v <= 64 * p, ("sum before its reduction", t, v / p)
        else:
            assert v <= 32 * p, ("value kept or forwarded", t, v / p)
    assert 0 <= out < p
    return out


def patterns(rng, p):
    rnd = {}

    def random_at(c, rot):
        return rnd.setdefault((c, rot), rng.randrange(p))
    return {"zero": lambda c, rot: 0, "max": lambda c, rot: p - 1,
            "alt0": lambda c, rot: 0 if (c + rot) % 2 == 0 else p - 1,
            "alt1": lambda c, rot: p - 1 if (c + rot) % 2 == 0 else 0, "random": random_at}


def var_settings(rng, p, n_vars):
    if n_vars == 0:
        return [[]]
    return [[0] * n_vars, [1] * n_vars, [p - 1] * n_vars, [rng.choice((0, 1, p - 1, rng.randrange(p))) for _ in range(n_vars)]]


def n_cols_of(nodes):
    return max([nd[1] for nd in nodes if nd[0] == COL], default=-1) + 1


def check_dag(lib, curve, nodes, consts, n_vars, rng):
    p = FIELDS[curve]
    rc, h = compile_public(lib, curve, nodes, consts, n_cols_of(nodes), n_vars)
    assert rc == 0
    prog = dump(lib, h, n_vars)
    assert lib.h2_expr_release(h) == 0
    reductions = reductions_of(prog)
    assert prog["table"].index(1) not in prog["var_slot"] and len(set(prog["var_slot"])) == n_vars
    for variables in var_settings(rng, p, n_vars):
        cw = working_table(prog, variables, p)
        for name, column_at in patterns(rng, p).items():
            got = check_row(p, prog["code"], cw, column_at, reductions)
            assert got == eval_dag(p, nodes, consts, variables, column_at) * (1 << 256) % p, (name, variables[:1])
    return prog


def random_dag(rng, p, n, n_cols, n_vars, n_consts=4, rots=(0, 1, -1, 7, -7)):
    """n nodes: a quarter leaves (columns at rotations, constants, variables), the rest add / sub / mul of earlier nodes,
    mostly recent ones (depth) and some anywhere (shared subexpressions)"""
    consts = [rng.choice((0, p - 1, rng.randrange(p), rng.randrange(p))) for _ in range(n_consts)]     # no 1: reductions_of
    nodes = []
    for _ in range(max(2, n // 4)):
        u = rng.random()
        if u < 0.6 or (n_vars == 0 and u < 0.8):
            nodes.append((COL, rng.randrange(n_cols), 0, rng.choice(rots)))
        elif u < 0.8:
            nodes.append((VAR, 0, 0, rng.randrange(n_vars)))
        else:
            nodes.append((CONST, 0, 0, rng.randrange(n_consts)))
    nodes[0] = (COL, n_cols - 1, 0, 0)
    while len(nodes) < n:
        k = len(nodes)
        a = rng.randrange(max(0, k - 4), k) if rng.random() < 0.7 else rng.randrange(k)
        b = rng.randrange(k)
        nodes.append((rng.choice((ADD, SUB, MUL, MUL)), a, b, 0))
    return nodes, consts


def chain_dags(p):
    """the adversarial sums, differences and products of test_expr_program.py with this field's p - 1, long product
    chains and squares of squares, and the same with variables at the leaves"""
    out = [(name, nodes, [p - 1] * len(consts), 0) for name, nodes, consts, _ in T.adversarial_dags()]
    for length in (40, 64):
        out.append(("prod%d" % length, T.chain(MUL, length), [], 0))
        out.append(("squares%d" % length, [(COL, 0, 0, 0)] + [(MUL, j, j, 0) for j in range(length)], [], 0))
    for op, name in ((ADD, "varsum"), (SUB, "vardiff"), (MUL, "varprod")):
        nodes = [(VAR, 0, 0, c % 3) if c % 2 else (COL, c, 0, 0) for c in range(40)]
        acc = 0
        for c in range(1, 40):
            nodes.append((op, acc, c, 0))
            acc = len(nodes) - 1
        out.append((name, nodes, [], 3))
    return out


@pytest.mark.parametrize("curve", [0, 1, 2])
def test_random_dags_with_variables(lib, curve):
    rng = random.Random(0xE7 + curve)
    for n in (5, 6, 9, 17, 33, 64, 120, 200, 300):
        for n_vars in (0, 3):
            nodes, consts = random_dag(rng, FIELDS[curve], n, 6, n_vars)
            check_dag(lib, curve, nodes, consts, n_vars, rng)


@pytest.mark.parametrize("curve", [0, 1, 2])
def test_sum_difference_and_product_chains(lib, curve):
    rng = random.Random(0xAD + curve)
    reduced = 0
    for name, nodes, consts, n_vars in chain_dags(FIELDS[curve]):
        reduced += check_dag(lib, curve, nodes, consts, n_vars, rng)["stats"][5]
    assert reduced > 0


@pytest.mark.parametrize("curve", [0, 1, 2])
def test_a_leaf_root_is_multiplied_by_one(lib, curve):
    rng = random.Random(curve)
    p = FIELDS[curve]
    for nodes, consts, n_vars in (([(COL, 0, 0, 0)], [], 0), ([(COL, 0, 0, 0), (COL, 1, 0, -3)], [], 0),
                                  ([(VAR, 0, 0, 1)], [], 2), ([(CONST, 0, 0, 0)], [p - 1], 0),
                                  ([(COL, 0, 0, 0), (CONST, 0, 0, 0)], [1], 0)):
        prog = check_dag(lib, curve, nodes, consts, n_vars, rng)
        assert prog["stats"][:2] == (1, 1)


def test_bn256_code_is_what_the_provers_compiler_emits(lib):
    rng = random.Random(0xB7)
    dags = [T.random_dag(rng, n, ncols=6) for n in (5, 17, 64, 200, 300)]
    dags += [(nodes, consts) for _, nodes, consts, _ in T.adversarial_dags()]
    for nodes, consts in dags:
        rc, want = T.compile_dag(lib, nodes, consts)
        assert rc == 0
        rc, h = compile_public(lib, 0, nodes, consts, n_cols_of(nodes), 0)
        assert rc == 0
        got = dump(lib, h, 0)
        assert lib.h2_expr_release(h) == 0
        assert (got["stats"], got["code"], got["table"]) == (want["stats"], want["code"], want["table"])


def test_info_reports_the_program(lib):
    nodes = [(COL, 0, 0, -5), (COL, 2, 0, 9), (VAR, 0, 0, 0), (MUL, 0, 1, 0), (ADD, 3, 2, 0)]
    rc, h = compile_public(lib, 1, nodes, [], 3, 1)
    assert rc == 0
    i, prog = info(lib, h), dump(lib, h, 1)
    assert (i.curve, i.n_cols, i.n_vars, i.min_rot, i.max_rot) == (1, 3, 1, -5, 9)
    assert (i.instructions, i.products, i.column_reads, i.slots, i.constants, i.reductions) == prog["stats"]
    assert i.lds_bytes == T.SLOT_BYTES and i.instructions == 2
    assert lib.h2_expr_release(h) == 0
    assert lib.h2_expr_release(h) == EHANDLE
