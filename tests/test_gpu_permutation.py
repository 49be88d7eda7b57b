"""GPU: h2_permutation_product_device -- the permutation argument's grand products of every set of every instance in one
call, each set started on the device at the last usable value of the set before it (csrc/h2_permutation.hpp).

The judge is pure-Python big integers with the primes of halo2_prover_amd/domain.py and needs no inversion: it checks the
recurrence by cross-multiplication, z_0[0] = 1, z_{s+1}[0] = z_s[u], z_s[i+1] den_s[i] == z_s[i] num_s[i], and
z_s[i+1] == 0 where den_s[i] == 0 -- which determines every value.  Outputs are pattern-filled buffers with padding rows
behind every column and tail rows behind the last: everything outside rows [0, u] must still hold the pattern, and every
result must be canonical.  Shapes are sized by T = h2_permutation_tile()."""
import ctypes
import hashlib
import os
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CID = {"bn254": 0, "pallas": 1, "vesta": 2}
H2_OK, H2_EINVAL = 0, -1
PATTERN = 0x5A5A5A5A5A5A5A5A
PATTERN_INT = int.from_bytes(b"\x5a" * 32, "little")
PAD, TAIL = 7, 3          # col_stride = u + 1 + PAD; TAIL pattern rows behind the last column
SCAN_MAX_JOBS = 8         # csrc/h2_poly.hpp
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def L():
    from halo2_prover_amd import lib
    return lib.load()


def tile():
    return L().h2_permutation_tile()


def field(curve):
    """(p, omega of order 2^20, delta = generator^(2^two-adicity)) of the curve's scalar field"""
    from halo2_prover_amd.domain import _FIELDS
    p, gen, S, _ = _FIELDS[CID[curve]]
    root = pow(gen, (p - 1) >> S, p)
    return p, pow(root, 1 << (S - 20), p), pow(gen, 1 << S, p)


def mont(p, values):
    R = (1 << 256) % p
    buf = b"".join((v * R % p).to_bytes(32, "little") for v in values)
    return np.frombuffer(buf, dtype=np.uint64).reshape(-1, 4).copy()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).cuda()


def limbs(p, v):
    return (ctypes.c_uint64 * 4)(*[int(x) for x in mont(p, [v])[0]])


def limbs_many(p, vs):
    return (ctypes.c_uint64 * (4 * len(vs)))(*[int(x) for x in mont(p, vs).reshape(-1)])


def blank(cols, stride):
    import torch
    return torch.full((cols * stride + TAIL, 4), PATTERN, dtype=torch.int64, device="cuda")


def upload(p, vals, sig):
    """every column in an allocation of its own"""
    return [[dev(mont(p, c)) for c in inst] for inst in vals], [dev(mont(p, c)) for c in sig]


def raw_call(curve, vptrs, sptrs, n_cols, chunk, u, m, betas, gammas, omega, delta, zptr, stride, stream=None):
    p = field(curve)[0]
    va = (ctypes.c_void_p * max(1, len(vptrs)))(*vptrs)
    sa = (ctypes.c_void_p * max(1, len(sptrs)))(*sptrs)
    return L().h2_permutation_product_device(CID[curve], va, sa, n_cols, chunk, u, m, limbs_many(p, betas), limbs_many(p, gammas),
                                             limbs(p, omega), limbs(p, delta), ctypes.c_void_p(zptr), stride, stream)


def call(curve, dv, ds, chunk, u, betas, gammas):
    """the raw call on device columns -> the z tensor (m * S columns of stride u + 1 + PAD, then TAIL rows)"""
    p, omega, delta = field(curve)
    m, n_cols = len(dv), len(ds)
    S = (n_cols + chunk - 1) // chunk
    z = blank(m * S, u + 1 + PAD)
    st = raw_call(curve, [c.data_ptr() for inst in dv for c in inst], [c.data_ptr() for c in ds], n_cols, chunk, u, m, betas, gammas,
                  omega, delta, z.data_ptr(), u + 1 + PAD)
    assert st == H2_OK, L().h2_last_device_error()
    return z


def read_back(curve, z, cols, u):
    """-> `cols` canonical columns of u + 1 values; every other row must still hold the pattern"""
    import torch
    torch.cuda.synchronize()
    p = field(curve)[0]
    rinv = pow((1 << 256) % p, -1, p)
    stride = u + 1 + PAD
    buf = z.cpu().numpy().tobytes()
    raw = [int.from_bytes(buf[i:i + 32], "little") for i in range(0, len(buf), 32)]
    out = []
    for c in range(cols):
        col = raw[c * stride:c * stride + u + 1]
        assert all(v < p for v in col), "a result is not canonical"
        assert all(v == PATTERN_INT for v in raw[c * stride + u + 1:(c + 1) * stride]), "rows behind row u were written"
        out.append([v * rinv % p for v in col])
    assert all(v == PATTERN_INT for v in raw[cols * stride:]), "memory behind the last column was written"
    return out


def judge(curve, vals, sig, chunk, u, beta, gamma, zcols):
    """one instance: its S columns against the recurrence, by cross-multiplication.  -> the tails z_s[u]"""
    p, omega, delta = field(curve)
    n_cols = len(sig)
    S = (n_cols + chunk - 1) // chunk
    assert len(zcols) == S
    bd = [beta * pow(delta, j, p) % p for j in range(n_cols)]
    prev = 1
    for s in range(S):
        z = zcols[s]
        assert z[0] == prev, "set %d does not start at the tail of the set before" % s
        w = 1
        for i in range(u):
            num = den = 1
            for j in range(s * chunk, min((s + 1) * chunk, n_cols)):
                num = num * (vals[j][i] + bd[j] * w + gamma) % p
                den = den * (vals[j][i] + beta * sig[j][i] + gamma) % p
            if den == 0:
                assert z[i + 1] == 0, "a zero denominator must give ratio 0 (set %d, row %d)" % (s, i)
            else:
                assert z[i + 1] * den % p == z[i] * num % p, "set %d, row %d" % (s, i)
            w = w * omega % p
        prev = z[u]
    return [zc[u] for zc in zcols]


def random_columns(rng, p, count, u):
    return [[rng.randrange(p) for _ in range(u)] for _ in range(count)]


def check(curve, vals, sig, chunk, u, betas, gammas):
    p = field(curve)[0]
    dv, ds = upload(p, vals, sig)
    m, S = len(vals), (len(sig) + chunk - 1) // chunk
    cols = read_back(curve, call(curve, dv, ds, chunk, u, betas, gammas), m * S, u)
    return [judge(curve, vals[q], sig, chunk, u, betas[q], gammas[q], cols[q * S:(q + 1) * S]) for q in range(m)], cols


# ---- 1. row edges ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", sorted(CID))
@pytest.mark.parametrize("tag", ["1", "2", "3", "4", "5", "T-1", "T", "T+1", "3T+5"])
def test_row_edges(h2, curve, tag):
    """n_cols = 3 in sets of 2 (a ragged last set), two instances with their own beta and gamma, every value column in an
    allocation of its own; u around the run of one thread and around the tile of one workgroup"""
    T = tile()
    u = {"T-1": T - 1, "T": T, "T+1": T + 1, "3T+5": 3 * T + 5}.get(tag) or int(tag)
    p = field(curve)[0]
    rng = random.Random("edges %s %s" % (curve, tag))
    vals = [random_columns(rng, p, 3, u) for _ in range(2)]
    sig = random_columns(rng, p, 3, u)
    check(curve, vals, sig, 2, u, [rng.randrange(p), rng.randrange(p)], [rng.randrange(p), rng.randrange(p)])


# ---- 2. copy constraints and chaining ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", sorted(CID))
def test_copy_constraints_close_the_product(h2, curve):
    """values constant on the cycles of a random permutation of the cells (j, i): the last set's tail is exactly 1 and the
    tails of the sets before it are not; with one value broken the last tail is not 1 either"""
    p, omega, delta = field(curve)
    n_cols, chunk, u = 5, 2, 37
    rng = random.Random("cycles " + curve)
    cells = [(j, i) for j in range(n_cols) for i in range(u)]
    image = cells[:]
    rng.shuffle(image)
    perm = dict(zip(cells, image))
    vals = [[None] * u for _ in range(n_cols)]
    for start in cells:
        if vals[start[0]][start[1]] is None:
            v, c = rng.randrange(p), start
            while vals[c[0]][c[1]] is None:
                vals[c[0]][c[1]] = v
                c = perm[c]
    sig = [[pow(delta, perm[(j, i)][0], p) * pow(omega, perm[(j, i)][1], p) % p for i in range(u)] for j in range(n_cols)]
    beta, gamma = rng.randrange(p), rng.randrange(p)
    (tails,), _ = check(curve, [vals], sig, chunk, u, [beta], [gamma])
    assert tails[-1] == 1
    assert all(t != 1 for t in tails[:-1])
    vals[3][11] = (vals[3][11] + 1) % p
    (tails,), _ = check(curve, [vals], sig, chunk, u, [beta], [gamma])
    assert tails[-1] != 1


# ---- 3. zero denominators ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("also_numerator", [False, True])
@pytest.mark.parametrize("where", ["in the first tile", "in the second tile"])
def test_zero_denominator(h2, where, also_numerator):
    """a zero denominator at one row of the middle set of instance 0 (with and without a zero numerator in the same row):
    the rows up to it follow the recurrence, every later row of that instance -- in that set and in the next -- is 0, and
    instance 1 is untouched"""
    curve = "bn254"
    p, omega, delta = field(curve)
    T = tile()
    u, r = (37, 18) if where == "in the first tile" else (T + 9, T + 2)
    n_cols, chunk = 5, 2
    rng = random.Random("zero %s %d" % (where, also_numerator))
    vals = [random_columns(rng, p, n_cols, u) for _ in range(2)]
    sig = random_columns(rng, p, n_cols, u)
    betas, gammas = [rng.randrange(1, p), rng.randrange(1, p)], [rng.randrange(p), rng.randrange(p)]
    vals[0][2][r] = -(betas[0] * sig[2][r] + gammas[0]) % p                      # column 2 of set 1 = {2, 3}
    if also_numerator:
        vals[0][3][r] = -(betas[0] * pow(delta, 3, p) * pow(omega, r, p) + gammas[0]) % p
    tails, cols = check(curve, vals, sig, chunk, u, betas, gammas)
    assert cols[0][u] != 0 and cols[1][r] != 0, "the rows before the planted one are alive"
    assert all(v == 0 for v in cols[1][r + 1:]) and all(v == 0 for v in cols[2])
    assert all(v != 0 for q in (3, 4, 5) for v in cols[q]), "the other instance is unaffected"


# ---- 4. scan geometry past 4096 chunks of 16 -----------------------------------------------------------------------------------
@pytest.mark.parametrize("u", [21862, 21850])
def test_scan_chunks_grow_and_straddle_sets(h2, u):
    """S u just past 65536: the scan's chunks are 17 elements long.  u = 21862 = 17 * 1286 keeps every chunk inside one
    set; u = 21850 is no multiple of 17, so chunks straddle the two set boundaries"""
    curve = "bn254"
    p = field(curve)[0]
    assert 3 * u > 4096 * 16 and (u % 17 == 0) == (u == 21862)
    rng = random.Random("scan %d" % u)
    vals = [random_columns(rng, p, 3, u)]
    sig = random_columns(rng, p, 3, u)
    check(curve, vals, sig, 1, u, [rng.randrange(p)], [rng.randrange(p)])


# ---- 5. group edges ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [SCAN_MAX_JOBS + 1, 257])
def test_more_instances_than_one_group(h2, m):
    """m = 9 is one more than the batched scan's SCAN_MAX_JOBS; m = 257 one more than this call's own scan group"""
    curve = "pallas"
    p = field(curve)[0]
    rng = random.Random("groups %d" % m)
    u = 6
    sig = random_columns(rng, p, 3, u)
    vals = [random_columns(rng, p, 3, u) for _ in range(m)]
    check(curve, vals, sig, 2, u, [rng.randrange(p) for _ in range(m)], [rng.randrange(p) for _ in range(m)])


def test_one_call_gives_the_bytes_of_one_call_per_instance(h2):
    curve = "vesta"
    p = field(curve)[0]
    rng = random.Random("grouping")
    u, m = tile() + 3, 3
    vals = [random_columns(rng, p, 3, u) for _ in range(m)]
    sig = random_columns(rng, p, 3, u)
    betas, gammas = [rng.randrange(p) for _ in range(m)], [rng.randrange(p) for _ in range(m)]
    dv, ds = upload(p, vals, sig)
    together = call(curve, dv, ds, 2, u, betas, gammas)
    read_back(curve, together, 2 * m, u)
    stride = u + 1 + PAD
    whole = together.cpu().numpy()
    for q in range(m):
        alone = call(curve, [dv[q]], ds, 2, u, [betas[q]], [gammas[q]])
        read_back(curve, alone, 2, u)
        assert alone.cpu().numpy()[:2 * stride].tobytes() == whole[2 * q * stride:2 * (q + 1) * stride].tobytes()


def test_repeated_pointers(h2):
    """one column twice within a set, and the same columns for both instances"""
    curve = "bn254"
    p = field(curve)[0]
    rng = random.Random("repeats")
    u = 21
    a, b = random_columns(rng, p, 2, u)
    sig = random_columns(rng, p, 3, u)
    dv, ds = upload(p, [[a, b]], sig)
    da, db = dv[0]
    betas, gammas = [rng.randrange(p), rng.randrange(p)], [rng.randrange(p), rng.randrange(p)]
    cols = read_back(curve, call(curve, [[da, da, db], [da, da, db]], ds, 2, u, betas, gammas), 4, u)
    for q in range(2):
        judge(curve, [a, a, b], sig, 2, u, betas[q], gammas[q], cols[2 * q:2 * q + 2])


# ---- 6. degenerate shapes ----------------------------------------------------------------------------------------------------
def test_degenerate_shapes(h2):
    import torch
    curve = "bn254"
    p, omega, delta = field(curve)
    one = dev(mont(p, [5]))
    # u = 0: z_s[0] = 1 for every column, nothing else
    z = call(curve, [[one, one, one], [one, one, one]], [one, one, one], 2, 0, [3, 4], [5, 6])
    assert read_back(curve, z, 4, 0) == [[1]] * 4
    # u = 0 needs no readable source column at all
    z = blank(2, 1 + PAD)
    assert raw_call(curve, [0, 0, 0], [0, 0, 0], 3, 2, 0, 1, [3], [5], omega, delta, z.data_ptr(), 1 + PAD) == H2_OK
    assert read_back(curve, z, 2, 0) == [[1]] * 2
    # n_cols = 0 and m = 0: H2_OK and nothing written, whatever the other arguments
    z = blank(2, 8 + PAD)
    assert raw_call(curve, [], [], 0, 2, 7, 2, [3, 4], [5, 6], omega, delta, z.data_ptr(), 8 + PAD) == H2_OK
    assert raw_call(curve, [], [], 0, 0, 7, 2, [3, 4], [5, 6], omega, delta, z.data_ptr(), 8 + PAD) == H2_OK
    assert raw_call(curve, [], [one.data_ptr()], 1, 1, 7, 0, [3], [5], omega, delta, z.data_ptr(), 8 + PAD) == H2_OK
    assert L().h2_permutation_product_device(0, None, None, 3, 2, 7, 0, None, None, None, None, None, 8, None) == H2_OK
    torch.cuda.synchronize()
    assert bool((z == PATTERN).all())


# ---- 7. argument errors ------------------------------------------------------------------------------------------------------
def test_invalid_arguments_enqueue_nothing(h2):
    import torch
    curve = "bn254"
    p, omega, delta = field(curve)
    rng = random.Random("errors")
    u, n_cols, chunk, m = 9, 3, 2, 2
    stride = u + 1 + PAD
    dv, ds = upload(p, [random_columns(rng, p, n_cols, u) for _ in range(m)], random_columns(rng, p, n_cols, u))
    vp, sp = [c.data_ptr() for inst in dv for c in inst], [c.data_ptr() for c in ds]
    z = blank(m * 2, stride)
    betas, gammas = [3, 4], [5, 6]
    b, g, w, d = limbs_many(p, betas), limbs_many(p, gammas), limbs(p, omega), limbs(p, delta)
    va, sa = (ctypes.c_void_p * len(vp))(*vp), (ctypes.c_void_p * len(sp))(*sp)
    zp = ctypes.c_void_p(z.data_ptr())
    fn = L().h2_permutation_product_device
    good = [0, va, sa, n_cols, chunk, u, m, b, g, w, d, zp, stride, None]

    def bad(**change):
        args = list(good)
        names = ["curve", "values", "sigma", "n_cols", "chunk", "u", "m", "beta", "gamma", "omega", "delta", "z", "stride", "stream"]
        for k, v in change.items():
            args[names.index(k)] = v
        assert fn(*args) == H2_EINVAL, change

    def with_entry(ptrs, at, value):
        q = list(ptrs)
        q[at] = value
        return (ctypes.c_void_p * len(q))(*q)

    bad(curve=7)
    bad(chunk=0)
    bad(u=(1 << 26) + 1, stride=(1 << 26) + 2)
    bad(stride=u)
    bad(stride=1 << 57)                                    # m S col_stride = 2^59
    bad(stride=(1 << 55) + 1)                              # just past 2^57
    for name in ("values", "sigma", "beta", "gamma", "omega", "delta", "z"):
        bad(**{name: None})
    bad(z=ctypes.c_void_p(z.data_ptr() + 8))
    bad(values=with_entry(vp, 4, None))
    bad(values=with_entry(vp, 4, vp[4] + 8))
    bad(sigma=with_entry(sp, 2, None))
    bad(sigma=with_entry(sp, 2, sp[2] + 8))
    # the output range over rows [0, u) of a source column: a value column of the last instance, a sigma column
    bad(values=with_entry(vp, 5, z.data_ptr() + 32 * (3 * stride + 2)))
    bad(sigma=with_entry(sp, 0, z.data_ptr() + 32 * (stride - 1)))
    bad(z=ctypes.c_void_p(vp[1] + 32 * (u - 1)))
    torch.cuda.synchronize()
    assert bool((z == PATTERN).all())
    for t in [c for inst in dv for c in inst] + ds:
        assert t.shape[0] == u
    # and the same arguments unchanged are accepted
    assert fn(*good) == H2_OK
    read_back(curve, z, 4, u)


# ---- the Python layer and the prover --------------------------------------------------------------------------------------------
def test_python_layer_matches_the_judge(h2):
    import torch
    from halo2_prover_amd.domain import EvaluationDomain
    dom = EvaluationDomain(3, 6, "pallas")
    p, _, delta = field("pallas")
    rng = random.Random("python layer")
    u, n_cols, chunk, m = dom.n - 6, 4, 3, 2
    vals = [random_columns(rng, p, n_cols, dom.n) for _ in range(m)]
    sig = random_columns(rng, p, n_cols, dom.n)
    dv, ds = upload(p, vals, sig)
    betas, gammas = [rng.randrange(p) for _ in range(m)], [rng.randrange(p) for _ in range(m)]
    z = h2.permutation_product(dom, dv, ds, chunk, u, betas, gammas, dom.omega, delta)
    assert tuple(z.shape) == (m, 2, dom.n, 4)
    torch.cuda.synchronize()
    rinv = pow((1 << 256) % p, -1, p)
    buf = z.cpu().numpy().tobytes()
    raw = [int.from_bytes(buf[i:i + 32], "little") for i in range(0, len(buf), 32)]
    bd = lambda q, j: betas[q] * pow(delta, j, p) % p
    for q in range(m):
        prev = 1
        for s in range(2):
            col = raw[(2 * q + s) * dom.n:(2 * q + s + 1) * dom.n]
            assert all(v == 0 for v in col[u + 1:])
            zc = [v * rinv % p for v in col[:u + 1]]
            assert zc[0] == prev
            for i in range(u):
                num = den = 1
                for j in range(s * chunk, min((s + 1) * chunk, n_cols)):
                    num = num * (vals[q][j][i] + bd(q, j) * pow(dom.omega, i, p) + gammas[q]) % p
                    den = den * (vals[q][j][i] + betas[q] * sig[j][i] + gammas[q]) % p
                assert den and zc[i + 1] * den % p == zc[i] * num % p
            prev = zc[u]


def test_the_prover_builds_its_grand_products_in_one_call(h2, monkeypatch):
    """a Poseidon k = 6 proof: h2_permutation_product_device exactly once, h2_poly_prefix_product_device not at all, and
    the recorded proof bytes"""
    import pyref as R
    from halo2_prover_amd import prover

    class SurveyRng:
        def __init__(self, start):
            self.s = R.SurveyStream(start=start)

        def fill(self, n):
            return self.s.fill(n)

        def fr_random(self, _field=None):
            return self.s.fr_random(R.BN_FR)

    params = h2.ParamsKZG.read(open(os.path.join(GOLDEN, "params_k6.bin"), "rb").read())
    circuit = prover.PoseidonCircuit([1, 2])
    pk = prover.generate_keys(params, circuit)
    lib = L()
    calls = {"h2_permutation_product_device": 0, "h2_poly_prefix_product_device": 0}

    def counting(name):
        fn = getattr(lib, name)

        def wrapper(*args):
            calls[name] += 1
            return fn(*args)
        return wrapper

    for name in calls:
        monkeypatch.setattr(lib, name, counting(name))
    proof = prover.generate_proof_with_instance(params, pk, circuit, [circuit.output()], SurveyRng(8))
    assert calls == {"h2_permutation_product_device": 1, "h2_poly_prefix_product_device": 0}
    assert hashlib.sha256(proof).hexdigest() == "6d235bf4637e1dce12559c44eaf77812bae2746d78331db3850e16b26234e63e"
    assert proof == open(os.path.join(GOLDEN, "proof_poseidon_k6.bin"), "rb").read()
