"""GPU: h2_lookup_permute_device / h2_lookup_product_device -- the lookup argument's permute_expression_pair and
commit_product over columns resident in HBM (csrc/h2_lookup.hpp).

The judge is a pure-Python big-integer transcription of the loop include/h2hip.h restates (sorted, a dict walked in
sorted key order, list.pop()) and of the grand product's recurrence, on canonical integers converted from and to
Montgomery form with the primes of halo2_prover_amd/domain.py.  Equal keys are indistinguishable, so A' and S' are unique
and every comparison is exact, on the raw Montgomery integers.  Lengths are sized by T = h2_lookup_tile(): the edges of a
wave, of a tile and of the scans across tiles."""
import ctypes
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CID = {"bn254": 0, "pallas": 1, "vesta": 2}
H2_OK, H2_EINVAL = 0, -1
PATTERN = 0x5A5A5A5A5A5A5A5A
PATTERN_INT = int.from_bytes(b"\x5a" * 32, "little")
STATUS_PATTERN = 0x5A5A5A5A
PAD, TAIL = 7, 3          # col_stride = u + PAD; TAIL pattern rows behind the last column


def L():
    from halo2_prover_amd import lib
    return lib.load()


def tile():
    return L().h2_lookup_tile()


def prime(curve):
    from halo2_prover_amd.domain import _FIELDS
    return _FIELDS[CID[curve]][0]


def raw_ints(a):
    buf = np.ascontiguousarray(a).tobytes()
    return [int.from_bytes(buf[i:i + 32], "little") for i in range(0, len(buf), 32)]


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).cuda()


def ptr(t, byte_offset=0):
    return ctypes.c_void_p(t.data_ptr() + byte_offset)


def columns(curve, cols, u, stride):
    """canonical columns (u values each) -> a device tensor of len(cols) * stride + TAIL rows of Montgomery limbs, the
    pattern everywhere outside rows [0, u) of every column"""
    p = prime(curve)
    R = (1 << 256) % p
    rows = [PATTERN_INT] * (len(cols) * stride + TAIL)
    for j, col in enumerate(cols):
        assert len(col) == u
        rows[j * stride:j * stride + u] = [v * R % p for v in col]
    buf = b"".join(v.to_bytes(32, "little") for v in rows)
    return dev(np.frombuffer(buf, dtype=np.uint64).reshape(-1, 4))


def blank(m, stride):
    import torch
    return torch.full((m * stride + TAIL, 4), PATTERN, dtype=torch.int64, device="cuda")


def read_back(curve, t, m, u, stride, rows=None):
    """-> m canonical columns of `rows` (default u) values; asserts that every other row still holds the pattern"""
    p = prime(curve)
    rinv = pow((1 << 256) % p, -1, p)
    rows = u if rows is None else rows
    raw = raw_ints(t.cpu().numpy().view(np.uint64))
    out = []
    for j in range(m):
        out.append([v * rinv % p for v in raw[j * stride:j * stride + rows]])
        assert all(v < p for v in raw[j * stride:j * stride + rows]), "a result is not canonical"
        assert all(v == PATTERN_INT for v in raw[j * stride + rows:(j + 1) * stride]), "rows behind the result were written"
    assert all(v == PATTERN_INT for v in raw[m * stride:]), "memory behind the last column was written"
    return out


def judge_permute(A, S):
    """the numbered loop of the issue / header on canonical integers -> (A', S'), S' = None for a failed pair"""
    u = len(A)
    Ap = sorted(A)
    left = {}
    for v in S:
        left[v] = left.get(v, 0) + 1
    Sp, rep = [0] * u, []
    for row in range(u):
        if row == 0 or Ap[row] != Ap[row - 1]:
            Sp[row] = Ap[row]
            if Ap[row] not in left:
                return Ap, None
            left[Ap[row]] -= 1
        else:
            rep.append(row)
    for value in sorted(left):
        for _ in range(left[value]):
            Sp[rep.pop()] = value
    assert not rep
    return Ap, Sp


def judge_product(p, A, S, Ap, Sp, beta, gamma):
    z = [1]
    for i in range(len(A)):
        den = (Ap[i] + beta) * (Sp[i] + gamma) % p
        ratio = (A[i] + beta) * (S[i] + gamma) * pow(den, -1, p) % p if den else 0
        z.append(z[-1] * ratio % p)
    return z


def permute(curve, inputs, tables, u, stream=None, d_in=None, d_tab=None):
    """raw call on m pairs of canonical columns -> (A' columns, S' columns, status list); layout checks included"""
    import torch
    m, stride = len(inputs), u + PAD
    d_in = columns(curve, inputs, u, stride) if d_in is None else d_in
    d_tab = columns(curve, tables, u, stride) if d_tab is None else d_tab
    pin, ptab = blank(m, stride), blank(m, stride)
    status = torch.full((m + 2,), STATUS_PATTERN, dtype=torch.int32, device="cuda")
    st = L().h2_lookup_permute_device(CID[curve], ptr(d_in), ptr(d_tab), u, stride, m, ptr(pin), ptr(ptab), ptr(status), stream)
    assert st == H2_OK, L().h2_last_device_error()
    return d_in, d_tab, pin, ptab, status


def finish_permute(curve, m, u, pin, ptab, status, failed=()):
    import torch
    torch.cuda.synchronize()
    stride = u + PAD
    words = [int(x) for x in status.cpu().numpy().view(np.uint32)]
    assert words[m:] == [STATUS_PATTERN] * 2, "status words beyond m were written"
    Ap = read_back(curve, pin, m, u, stride)
    if failed:      # the u rows of a failed pair's S' are unspecified: only the rows around them are checked
        raw = raw_ints(ptab.cpu().numpy().view(np.uint64))
        p = prime(curve)
        rinv = pow((1 << 256) % p, -1, p)
        Sp = [[v * rinv % p for v in raw[j * stride:j * stride + u]] for j in range(m)]
        for j in range(m):
            assert all(v == PATTERN_INT for v in raw[j * stride + u:(j + 1) * stride])
        assert all(v == PATTERN_INT for v in raw[m * stride:])
    else:
        Sp = read_back(curve, ptab, m, u, stride)
    return Ap, Sp, words[:m]


def check_pairs(curve, inputs, tables, u, stream=None):
    """permute the pairs, compare with the judge and check the properties that need no judge"""
    _, _, pin, ptab, status = permute(curve, inputs, tables, u, stream)
    Ap, Sp, words = finish_permute(curve, len(inputs), u, pin, ptab, status)
    assert words == [0] * len(inputs)
    for j, (A, S) in enumerate(zip(inputs, tables)):
        assert sorted(Ap[j]) == sorted(A) and sorted(Sp[j]) == sorted(S)
        assert all(Ap[j][i] == Sp[j][i] or (i > 0 and Ap[j][i] == Ap[j][i - 1]) for i in range(u))
        want_a, want_s = judge_permute(A, S)
        assert Ap[j] == want_a
        assert Sp[j] == want_s
    return Ap, Sp


def product(curve, tensors, u, m, beta, gamma, stream=None):
    """raw call on the device tensors (input, table, A', S') -> m canonical columns of u + 1 values"""
    import torch
    p = prime(curve)
    R = (1 << 256) % p
    stride = u + PAD
    z = blank(m, stride)
    b = np.frombuffer((beta * R % p).to_bytes(32, "little"), dtype=np.uint64).copy()
    g = np.frombuffer((gamma * R % p).to_bytes(32, "little"), dtype=np.uint64).copy()
    st = L().h2_lookup_product_device(CID[curve], *[ptr(t) for t in tensors], u, stride, m, b.ctypes.data, g.ctypes.data, ptr(z), stream)
    assert st == H2_OK, L().h2_last_device_error()
    torch.cuda.synchronize()
    return read_back(curve, z, m, u, stride, rows=u + 1)


def drawn_pair(p, rng, u, bits=254, distinct=None):
    """a table of u values below 2^bits (mod p) with a few duplicates and an input drawn from its values with repeats"""
    pool = [rng.getrandbits(bits) % p for _ in range(distinct or max(1, (3 * u) // 4))]
    table = [rng.choice(pool) for _ in range(u)]
    return [rng.choice(table) for _ in range(u)], table


# name -> (multiple of T, offset)
LENGTHS = {"0": (0, 0), "1": (0, 1), "2": (0, 2), "3": (0, 3), "63": (0, 63), "64": (0, 64), "65": (0, 65), "T-1": (1, -1),
           "T": (1, 0), "T+1": (1, 1), "2T+3": (2, 3), "5T-1": (5, -1)}


def length_of(tag, T):
    mult, off = LENGTHS[tag]
    return mult * T + off


@pytest.mark.parametrize("tag", list(LENGTHS))
@pytest.mark.parametrize("curve", ["bn254", "pallas", "vesta"])
def test_lengths(h2, curve, tag):
    """pair 0: 254-bit values (all 32 passes), pair 1: an 8-bit range (one pass); the product on BN254 at every length
    and on the Pasta fields at 2T+3"""
    p = prime(curve)
    u = length_of(tag, tile())
    rng = random.Random(0x100C ^ (u * 3 + CID[curve]))
    pairs = [drawn_pair(p, rng, u), drawn_pair(p, rng, u, bits=8)]
    inputs, tables = [a for a, _ in pairs], [s for _, s in pairs]
    d_in, d_tab, pin, ptab, status = permute(curve, inputs, tables, u)
    Ap, Sp, words = finish_permute(curve, 2, u, pin, ptab, status)
    assert words == [0, 0]
    for j in range(2):
        want_a, want_s = judge_permute(inputs[j], tables[j])
        assert Ap[j] == want_a
        assert Sp[j] == want_s
    if curve == "bn254" or tag == "2T+3":
        beta, gamma = rng.randrange(p), rng.randrange(p)
        z = product(curve, (d_in, d_tab, pin, ptab), u, 2, beta, gamma)
        for j in range(2):
            assert z[j] == judge_product(p, inputs[j], tables[j], Ap[j], Sp[j], beta, gamma)
            assert z[j][0] == 1 and z[j][u] == 1


def test_multi_workgroup_scans(h2):
    """u = 2^16 - 6 on BN254: 64 tiles, so the per-pass scan and the scans across tiles run over many entries"""
    p = prime("bn254")
    u = (1 << 16) - 6
    rng = random.Random(0x2E16)
    A, S = drawn_pair(p, rng, u)
    d_in, d_tab, pin, ptab, status = permute("bn254", [A], [S], u)
    Ap, Sp, words = finish_permute("bn254", 1, u, pin, ptab, status)
    want_a, want_s = judge_permute(A, S)
    assert words == [0] and Ap[0] == want_a and Sp[0] == want_s
    beta, gamma = rng.randrange(p), rng.randrange(p)
    z = product("bn254", (d_in, d_tab, pin, ptab), u, 1, beta, gamma)
    assert z[0] == judge_product(p, A, S, Ap[0], Sp[0], beta, gamma) and z[0][u] == 1


def shapes(p, u, rng):
    """name -> (input, table), every pair satisfiable"""
    out = {}
    v = rng.randrange(p)
    out["all-equal input, value once in the table"] = ([v] * u, [v] + [rng.randrange(p) for _ in range(u - 1)])
    t = rng.sample(range(1, 1 << 40), u)
    a = list(t)
    rng.shuffle(a)
    out["permutation of a duplicate-free table"] = (a, t)
    t = [v, v, v] + [rng.randrange(p) for _ in range(u - 3)]
    rng.shuffle(t)
    out["table value of multiplicity 3"] = ([rng.choice(t) for _ in range(u - 2)] + [v, v], t)
    base = rng.getrandbits(250)
    for name, variants in (("top limb only", [base ^ (k << 192) for k in range(1, 40)]),
                           ("bit 0 only", [base, base ^ 1]),
                           ("one middle byte only", [base ^ (k << 104) for k in range(256)])):
        t = [rng.choice(variants) for _ in range(u)]
        out["keys that differ in " + name] = ([rng.choice(t) for _ in range(u)], t)
    edge = [0, 1, p - 1, 1 << 64, 1 << 128, 1 << 192]
    t = edge + [rng.choice(edge) for _ in range(u - len(edge))]
    out["0, 1, p-1 and the limb edges"] = ([rng.choice(edge) for _ in range(u)], t)
    t = list(range(256)) + [0] * (u - 256)            # canonical order versus the order of the Montgomery limbs
    out["8-bit range table"] = ([rng.randrange(256) for _ in range(u)], t)
    out["random 254-bit values"] = drawn_pair(p, rng, u)
    return out


SHAPE_NAMES = list(shapes(prime("bn254"), 300, random.Random(0)))


@pytest.mark.parametrize("name", SHAPE_NAMES)
def test_value_shapes(h2, name):
    p = prime("bn254")
    u = 2 * tile() + 3
    A, S = shapes(p, u, random.Random(0x5A17))[name]
    check_pairs("bn254", [A], [S], u)


def test_failed_pair(h2):
    """m = 3, pair 1 has one input value that its table lacks: status [0, 1, 0], pairs 0 and 2 exact, pair 1's A' sorted"""
    p = prime("bn254")
    u = 2 * tile() + 3
    rng = random.Random(0xFA11)
    pairs = [drawn_pair(p, rng, u) for _ in range(3)]
    missing = next(v for v in iter(lambda: rng.randrange(p), None) if v not in set(pairs[1][1]))
    pairs[1][0][u // 2] = missing
    inputs, tables = [a for a, _ in pairs], [s for _, s in pairs]
    _, _, pin, ptab, status = permute("bn254", inputs, tables, u)
    Ap, Sp, words = finish_permute("bn254", 3, u, pin, ptab, status, failed=(1,))
    assert words == [0, 1, 0]
    assert judge_permute(inputs[1], tables[1])[1] is None
    assert Ap[1] == sorted(inputs[1])
    for j in (0, 2):
        assert (Ap[j], Sp[j]) == judge_permute(inputs[j], tables[j])


def test_side_stream_and_two_streams(h2):
    import torch
    p = prime("bn254")
    T = tile()
    rng = random.Random(0x57E4)
    u1, u2 = 2 * T + 3, T + 1
    A1, S1 = drawn_pair(p, rng, u1)
    A2, S2 = drawn_pair(p, rng, u2, bits=8)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    d1 = (columns("bn254", [A1], u1, u1 + PAD), columns("bn254", [S1], u1, u1 + PAD))
    d2 = (columns("bn254", [A2], u2, u2 + PAD), columns("bn254", [S2], u2, u2 + PAD))
    torch.cuda.synchronize()
    # one call on a side stream
    r = permute("bn254", [A1], [S1], u1, ctypes.c_void_p(s1.cuda_stream), *d1)
    Ap, Sp, words = finish_permute("bn254", 1, u1, *r[2:])
    assert words == [0] and (Ap[0], Sp[0]) == judge_permute(A1, S1)
    # two different calls on two streams, enqueued back to back
    ra = permute("bn254", [A1], [S1], u1, ctypes.c_void_p(s1.cuda_stream), *d1)
    rb = permute("bn254", [A2], [S2], u2, ctypes.c_void_p(s2.cuda_stream), *d2)
    Ap, Sp, words = finish_permute("bn254", 1, u1, *ra[2:])
    assert words == [0] and (Ap[0], Sp[0]) == judge_permute(A1, S1)
    Ap, Sp, words = finish_permute("bn254", 1, u2, *rb[2:])
    assert words == [0] and (Ap[0], Sp[0]) == judge_permute(A2, S2)


def test_product_zero_denominator(h2):
    """beta = -A'[r]: the denominator of every row holding that value is zero, the ratio there is 0 and z stays 0 from
    the first such row on"""
    p = prime("bn254")
    u = 2 * tile() + 3
    rng = random.Random(0x2E20)
    A, S = drawn_pair(p, rng, u)
    d_in, d_tab, pin, ptab, status = permute("bn254", [A], [S], u)
    Ap, Sp, _ = finish_permute("bn254", 1, u, pin, ptab, status)
    # a value whose first row in A' comes before its first row in A: the first zero factor is a denominator
    r = next(i for i in range(u // 3, u) if Ap[0].index(Ap[0][i]) < A.index(Ap[0][i]))
    beta, gamma = (p - Ap[0][r]) % p, rng.randrange(p)
    z = product("bn254", (d_in, d_tab, pin, ptab), u, 1, beta, gamma)
    assert z[0] == judge_product(p, A, S, Ap[0], Sp[0], beta, gamma)
    first = Ap[0].index(Ap[0][r])
    assert z[0][first] != 0 and all(v == 0 for v in z[0][first + 1:])


def test_m_zero_and_u_zero(h2):
    import torch
    stride = PAD
    pin, ptab, z = blank(2, stride), blank(2, stride), blank(2, stride)
    status = torch.full((4,), STATUS_PATTERN, dtype=torch.int32, device="cuda")
    one = np.array([1, 0, 0, 0], dtype=np.uint64)
    # m = 0: nothing is enqueued, null pointers are fine
    assert L().h2_lookup_permute_device(0, None, None, 5, 5, 0, None, None, None, None) == H2_OK
    assert L().h2_lookup_product_device(0, None, None, None, None, 5, 6, 0, None, None, None, None) == H2_OK
    # usable_rows = 0: m zero status words; z[0] = 1
    assert L().h2_lookup_permute_device(0, None, None, 0, stride, 2, ptr(pin), ptr(ptab), ptr(status), None) == H2_OK
    assert L().h2_lookup_product_device(0, None, None, None, None, 0, stride, 2, one.ctypes.data, one.ctypes.data, ptr(z), None) == H2_OK
    torch.cuda.synchronize()
    assert [int(x) for x in status.cpu().numpy().view(np.uint32)] == [0, 0, STATUS_PATTERN, STATUS_PATTERN]
    read_back("bn254", pin, 2, 0, stride)
    read_back("bn254", ptab, 2, 0, stride)
    assert read_back("bn254", z, 2, 0, stride, rows=1) == [[1], [1]]


def test_invalid_arguments_enqueue_nothing(h2):
    import torch
    p = prime("bn254")
    u, m = 70, 2
    stride = u + PAD
    rng = random.Random(0xE1A7)
    pairs = [drawn_pair(p, rng, u) for _ in range(m)]
    d_in = columns("bn254", [a for a, _ in pairs], u, stride)
    d_tab = columns("bn254", [s for _, s in pairs], u, stride)
    pin, ptab, z = blank(m, stride), blank(m, stride), blank(m, stride)
    status = torch.full((m + 2,), STATUS_PATTERN, dtype=torch.int32, device="cuda")
    one = np.array([1, 0, 0, 0], dtype=np.uint64)
    big = (1 << 26) + 1

    def perm(curve=0, a=ptr(d_in), s=ptr(d_tab), rows=u, cs=stride, oa=ptr(pin), os_=ptr(ptab), st=ptr(status)):
        return L().h2_lookup_permute_device(curve, a, s, rows, cs, m, oa, os_, st, None)

    def prod(curve=0, a=ptr(d_in), s=ptr(d_tab), pa=ptr(d_in), ps=ptr(d_tab), rows=u, cs=stride, b=one.ctypes.data,
             g=one.ctypes.data, out=ptr(z)):
        return L().h2_lookup_product_device(curve, a, s, pa, ps, rows, cs, m, b, g, out, None)

    cases = {
        "permute: unknown curve": perm(curve=7),
        "permute: null input": perm(a=None), "permute: null table": perm(s=None),
        "permute: null A'": perm(oa=None), "permute: null S'": perm(os_=None), "permute: null status": perm(st=None),
        "permute: misaligned input": perm(a=ptr(d_in, 8)), "permute: misaligned table": perm(s=ptr(d_tab, 8)),
        "permute: misaligned A'": perm(oa=ptr(pin, 8)), "permute: misaligned S'": perm(os_=ptr(ptab, 8)),
        "permute: misaligned status": perm(st=ptr(status, 2)),
        "permute: col_stride too small": perm(cs=u - 1),
        "permute: usable_rows > 2^26": perm(rows=big, cs=big),
        "permute: A' is the input": perm(oa=ptr(d_in)), "permute: S' overlaps the table": perm(os_=ptr(d_tab, 32 * (stride + 3))),
        "permute: S' overlaps A'": perm(os_=ptr(pin, 32 * (u - 1))), "permute: status inside A'": perm(st=ptr(pin, 64)),
        "product: unknown curve": prod(curve=7),
        "product: null input": prod(a=None), "product: null S'": prod(ps=None), "product: null z": prod(out=None),
        "product: null beta": prod(b=None), "product: null gamma": prod(g=None),
        "product: misaligned table": prod(s=ptr(d_tab, 8)), "product: misaligned z": prod(out=ptr(z, 8)),
        "product: col_stride too small": prod(cs=u),
        "product: usable_rows > 2^26": prod(rows=big, cs=big + 1),
        "product: z is the input": prod(out=ptr(d_in)), "product: z overlaps A'": prod(pa=ptr(z, 32 * (stride + 1))),
    }
    assert {k: v for k, v in cases.items() if v != H2_EINVAL} == {}
    torch.cuda.synchronize()
    for t in (pin, ptab, z):            # nothing was enqueued: the outputs still hold the pattern
        read_back("bn254", t, m, 0, stride)
    assert [int(x) for x in status.cpu().numpy().view(np.uint32)] == [STATUS_PATTERN] * (m + 2)


def test_python_layer_matches_the_raw_calls(h2):
    import torch
    from halo2_prover_amd.domain import EvaluationDomain
    from halo2_prover_amd.lookup import lookup_product, permute_expression_pair
    curve = "pallas"
    p = prime(curve)
    u, m = tile() + 1, 2
    stride = u + PAD
    rng = random.Random(0x9717)
    pairs = [drawn_pair(p, rng, u), drawn_pair(p, rng, u, bits=8)]
    inputs, tables = [a for a, _ in pairs], [s for _, s in pairs]
    d_in, d_tab, pin, ptab, status = permute(curve, inputs, tables, u)
    torch.cuda.synchronize()
    beta, gamma = rng.randrange(p), rng.randrange(p)
    z = product(curve, (d_in, d_tab, pin, ptab), u, m, beta, gamma)
    dom = EvaluationDomain(4, 4, curve)
    t_in, t_tab = (t[:m * stride].reshape(m, stride, 4).contiguous() for t in (d_in, d_tab))
    a2, s2, st2 = permute_expression_pair(dom, t_in, t_tab, u)
    z2 = lookup_product(dom, t_in, t_tab, a2, s2, u, beta, gamma)
    torch.cuda.synchronize()
    assert st2.dtype == torch.int32 and st2.tolist() == [0, 0]
    for mine, raw in ((a2, pin), (s2, ptab)):
        assert torch.equal(mine[:, :u], raw[:m * stride].reshape(m, stride, 4)[:, :u])
        assert int(mine[:, u:].abs().sum()) == 0
    rinv = pow((1 << 256) % p, -1, p)
    for j in range(m):
        assert [v * rinv % p for v in raw_ints(z2[j, :u + 1].cpu().numpy().view(np.uint64))] == z[j]
