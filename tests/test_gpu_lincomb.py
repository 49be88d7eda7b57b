"""GPU: h2_poly_lincomb_device -- linear combinations of columns resident in HBM, a remainder's low coefficients
subtracted and linear factors divided out (csrc/h2_poly.hpp: poly_lincomb_kernel and the scan kernels, mode 0).

The judge is Python big-integer arithmetic modulo the field's prime (the primes of halo2_prover_amd/domain.py).  It works
on the raw Montgomery integers: the sum, the subtraction and kate_division are linear in the data, so with columns a_t R,
low coefficients l R and TRUE coefficients c_t and points z the result's Montgomery integers are the same operations on
the raw integers.  The division is oracle/halo2_ref.py's pdiv_linear with a zero appended (restated here with the prime
as an argument, and held against the oracle's on BN254).  Both sides are canonical, so every comparison is exact.

Every call runs inside one device buffer in which red zones surround the sources and follow every output: whatever the
call was not asked to write must come back unchanged."""
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CID = {"bn254": 0, "pallas": 1, "vesta": 2}
CURVES = ["bn254", "pallas", "vesta"]
H2_OK, H2_EINVAL = 0, -1
PATTERN = 0x5A5A5A5A5A5A5A5A
RED = 8                                   # rows of PATTERN between two columns


def L():
    from halo2_prover_amd import lib
    return lib.load()


def max_rounds():
    return L().h2_poly_lincomb_max_rounds()


def prime(curve):
    from halo2_prover_amd.domain import _FIELDS
    return _FIELDS[CID[curve]][0]


def raw_limbs(values):
    """ints below 2^256 -> (len, 4) uint64"""
    buf = b"".join(v.to_bytes(32, "little") for v in values)
    return np.frombuffer(buf, dtype=np.uint64).reshape(-1, 4).copy()


def raw_ints(a):
    buf = np.ascontiguousarray(a).tobytes()
    return [int.from_bytes(buf[i:i + 32], "little") for i in range(0, len(buf), 32)]


def mont(p, values):
    R = (1 << 256) % p
    return raw_limbs([v % p * R % p for v in values])


def pdiv_linear(a, z, p):
    """oracle/halo2_ref.py pdiv_linear over the field of p elements"""
    q = [0] * (len(a) - 1)
    acc = 0
    for i in range(len(a) - 1, 0, -1):
        acc = (a[i] + acc * z) % p
        q[i - 1] = acc
    return q


def reference(p, columns, job, n):
    """job: dict(terms=[(coefficient, column index)], low=[raw ints], points=[ints])"""
    s = [0] * n
    for c, idx in job["terms"]:
        col = columns[idx]
        if c:
            s = [(x + c * y) % p for x, y in zip(s, col)]
    for i, l in enumerate(job.get("low", [])):
        s[i] = (s[i] - l) % p
    for z in job.get("points", []):
        s = pdiv_linear(s, z, p) + [0]
    return s


class Layout:
    """sources and outputs in ONE device buffer, RED rows of PATTERN before, between and behind them"""

    def __init__(self, columns, jobs, n):
        import torch
        self.n = n
        self.src_row, self.out_row = [], []
        row = RED
        for _ in columns:
            self.src_row.append(row)
            row += n + RED
        for job in jobs:
            if job.get("alias") is not None:
                self.out_row.append(self.src_row[job["alias"]])
            else:
                self.out_row.append(row)
                row += n + RED
        host = np.full((row, 4), PATTERN, dtype=np.uint64)
        for r, col in zip(self.src_row, columns):
            if n:
                host[r:r + n] = raw_limbs(col[:n])
        self.before = host
        self.buf = torch.from_numpy(host.view(np.int64).copy()).cuda()

    def ptr(self, row):
        return self.buf.data_ptr() + 32 * row

    def after(self):
        import torch
        torch.cuda.synchronize()
        return self.buf.cpu().numpy().view(np.uint64)

    def outputs(self):
        """the outputs as raw ints; everything else in the buffer must be as it was"""
        got = self.after()
        mask = np.ones(got.shape[0], dtype=bool)
        for r in self.out_row:
            mask[r:r + self.n] = False
        assert np.array_equal(got[mask], self.before[mask]), "the call wrote outside its outputs"
        return [raw_ints(got[r:r + self.n]) for r in self.out_row]


def tables(curve, lay, jobs):
    """the four host arrays of the call"""
    from halo2_prover_amd.opening import LincombJob, LincombTerm
    p = prime(curve)
    flat = [(c, idx) for job in jobs for c, idx in job["terms"]]
    terms = (LincombTerm * max(1, len(flat)))()
    cm = mont(p, [c for c, _ in flat]) if flat else None
    for t, (c, idx) in enumerate(flat):
        terms[t].d_poly = lay.ptr(lay.src_row[idx])
        terms[t].coeff[:] = [int(x) for x in cm[t]]
    table = (LincombJob * max(1, len(jobs)))()
    low, points, at = [], [], 0
    for j, job in enumerate(jobs):
        table[j].d_out = lay.ptr(lay.out_row[j])
        table[j].first_term, table[j].n_terms = at, len(job["terms"])
        at += len(job["terms"])
        table[j].first_low, table[j].n_low = len(low), len(job.get("low", []))
        low += job.get("low", [])
        table[j].first_point, table[j].n_points = len(points), len(job.get("points", []))
        points += job.get("points", [])
    lm = raw_limbs(low).reshape(-1) if low else np.zeros(4, dtype=np.uint64)
    pm = mont(p, points).reshape(-1) if points else np.zeros(4, dtype=np.uint64)
    return table, terms, len(flat), lm, len(low), pm, len(points)


def run(curve, columns, jobs, n):
    """-> the outputs of the jobs as raw ints, after ONE call"""
    lay = Layout(columns, jobs, n)
    table, terms, nt, lm, nl, pm, npts = tables(curve, lay, jobs)
    st = L().h2_poly_lincomb_device(CID[curve], table, len(jobs), terms, nt, lm.ctypes.data, nl, pm.ctypes.data, npts, n, None)
    assert st == H2_OK
    return lay.outputs()


def random_columns(p, rng, n, count):
    """random canonical columns; the last two are all p - 1 (the largest integer the lazy sum must carry) and all zero"""
    cols = [[rng.randrange(p) for _ in range(n)] for _ in range(max(0, count - 2))]
    return cols + [[p - 1] * n, [0] * n]


SIZES = [1, 2, 15, 16, 17, 257, 65536, 65537]      # the last two: either side of the scan's 4096 x 16 chunk boundary


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("curve", CURVES)
def test_sizes(h2, curve, n):
    p = prime(curve)
    rng = random.Random(0x4C494E43 ^ (n * 3 + CID[curve]))
    columns = random_columns(p, rng, n, 4)
    z = [rng.randrange(p) for _ in range(3)]
    low = [rng.randrange(p) for _ in range(n)]
    jobs = [
        {"terms": [(rng.randrange(p), 0), (p - 1, 1)], "low": low[:min(3, n)], "points": [z[0]]},
        {"terms": [(p - 1, 2)], "low": low, "points": []},
        {"terms": [(1, 0), (rng.randrange(p), 2), (rng.randrange(p), 1)], "low": low[:1], "points": [z[1], 0]},
        {"terms": [(rng.randrange(p), 1)], "points": [z[2], z[2], z[0]]},
    ]
    got = run(curve, columns, jobs, n)
    for j, job in enumerate(jobs):
        assert got[j] == reference(p, columns, job, n), "job %d" % j


def test_the_division_is_the_oracles(h2):
    """the restated pdiv_linear against oracle/halo2_ref.py's on BN254"""
    import halo2_ref
    p = prime("bn254")
    assert p == halo2_ref.P
    rng = random.Random(7)
    a, z = [rng.randrange(p) for _ in range(33)], rng.randrange(p)
    assert pdiv_linear(a, z, p) == halo2_ref.pdiv_linear(a, z)


# 31 .. 33 and 64, 65: either side of the fold of the lazy sum, every 32 terms
TERM_COUNTS = [0, 1, 2, 24, 25, 31, 32, 33, 64, 65, 70]


@pytest.mark.parametrize("count", TERM_COUNTS)
@pytest.mark.parametrize("curve", CURVES)
def test_term_counts(h2, curve, count):
    """repeated pointers, coefficients 0, 1, p - 1, every n_low and n_points; n = 300: two workgroups, the second partial"""
    p = prime(curve)
    n = 300
    rng = random.Random(0x5445524D ^ (count * 3 + CID[curve]))
    columns = random_columns(p, rng, n, 5)
    special = [0, 1, p - 1]
    R = max_rounds()

    def terms(shift):
        # the all-(p - 1) column with coefficient p - 1 over and over is the sum of largest magnitude
        return [((special[(t + shift) % 3] if (t + shift) % 4 else rng.randrange(p)), (t + shift) % 5) for t in range(count)]
    z = [rng.randrange(p) for _ in range(R)]
    low = [rng.randrange(p) for _ in range(n)]
    jobs = [
        {"terms": terms(0), "low": [], "points": []},
        {"terms": terms(1), "low": low[:1], "points": [z[0]]},
        {"terms": terms(2), "low": low[:3], "points": [z[1], 0]},
        {"terms": terms(3), "low": low, "points": [z[2], z[2], z[0]]},
        {"terms": [(p - 1, 3)] * count, "low": [], "points": z},
    ]
    got = run(curve, columns, jobs, n)
    for j, job in enumerate(jobs):
        assert got[j] == reference(p, columns, job, n), "job %d" % j


def poly_mul_linear(a, z, p):
    """a(X) (X - z)"""
    out = [0] * (len(a) + 1)
    for i, c in enumerate(a):
        out[i + 1] = (out[i + 1] + c) % p
        out[i] = (out[i] - c * z) % p
    return out


@pytest.mark.parametrize("curve", CURVES)
def test_exact_division(h2, curve):
    """a sum that vanishes on a 3-point set once its remainder is subtracted: the output times prod (X - z) is the sum
    minus low, as polynomials"""
    p = prime(curve)
    n = 777
    rng = random.Random(0x45584143 + CID[curve])
    columns = random_columns(p, rng, n, 4)
    terms = [(rng.randrange(p), 0), (rng.randrange(p), 1), (rng.randrange(p), 2)]
    s = reference(p, columns, {"terms": terms}, n)
    zs = [rng.randrange(p) for _ in range(3)]
    # the remainder of s by Z = prod (X - z): s - q Z for the floor quotient q (three divisions, remainders dropped)
    q = s
    for z in zs:
        q = pdiv_linear(q, z, p) + [0]
    qz = q[:n - 3]
    for z in zs:
        qz = poly_mul_linear(qz, z, p)
    rem = [(a - b) % p for a, b in zip(s, qz)]
    assert not any(rem[3:])
    got = run(curve, columns, [{"terms": terms, "low": rem[:3], "points": zs}], n)[0]
    assert got[n - 3:] == [0, 0, 0]
    back = got[:n - 3]
    for z in zs:
        back = poly_mul_linear(back, z, p)
    want = list(s)
    for i in range(3):
        want[i] = (want[i] - rem[i]) % p
    assert back == want
    for z in zs:                      # and the sum minus low does vanish there
        acc = 0
        for c in reversed(want):
            acc = (acc * z + c) % p
        assert acc == 0


@pytest.mark.parametrize("count", [1, 8, 9, 17])
@pytest.mark.parametrize("curve", CURVES)
def test_dividing_jobs_side_by_side(h2, curve, count):
    """jobs with DIFFERENT n_points in one call: each output bit-equal to the same job run alone, and to the judge"""
    p = prime(curve)
    n = 1000
    rng = random.Random(0x53494445 ^ (count * 3 + CID[curve]))
    columns = random_columns(p, rng, n, 5)
    R = max_rounds()
    jobs = []
    for j in range(count):
        k = 1 + (j * 2) % R if j % 5 else R
        jobs.append({"terms": [(rng.randrange(p), (j + t) % 5) for t in range(1 + j % 4)],
                     "low": [rng.randrange(p) for _ in range(min(k, 3))],
                     "points": [rng.randrange(p) for _ in range(k)]})
    if count >= 9:
        jobs.insert(4, {"terms": [(rng.randrange(p), 0)], "points": []})     # one that divides nothing, among them
    assert len({len(j["points"]) for j in jobs}) > 1 or count == 1
    together = run(curve, columns, jobs, n)
    for j, job in enumerate(jobs):
        assert together[j] == reference(p, columns, job, n), "job %d" % j
    for j in sorted({0, len(jobs) // 2, len(jobs) - 1}):
        assert run(curve, columns, [jobs[j]], n)[0] == together[j], "job %d alone" % j


def test_groups_share_the_scratch(h2):
    """more dividing jobs than one group's intermediate columns hold (256 MiB of n * 32 bytes): the groups run one after
    another over the same scratch, and a job's bits do not depend on its group"""
    curve, n = "bn254", 1 << 16
    p = prime(curve)
    per_group = (256 << 20) // (n * 32)
    count = per_group + 2
    rng = random.Random(0x47525053)
    columns = [[rng.randrange(p) for _ in range(n)]]
    jobs = [{"terms": [(rng.randrange(p), 0)], "points": [rng.randrange(p)] * (1 + j % 2)} for j in range(count)]
    together = run(curve, columns, jobs, n)
    for j in (0, per_group - 1, per_group, count - 1):
        assert together[j] == reference(p, columns, jobs[j], n), "job %d" % j


@pytest.mark.parametrize("curve", CURVES)
def test_output_aliases_a_term(h2, curve):
    """n_points = 0: d_out may be one of the job's own term columns, even one that repeats"""
    p = prime(curve)
    n = 513
    rng = random.Random(0x414C4941 + CID[curve])
    columns = random_columns(p, rng, n, 4)
    job = {"terms": [(rng.randrange(p), 1), (rng.randrange(p), 0), (p - 1, 1)], "low": [rng.randrange(p)], "points": [],
           "alias": 1}
    other = {"terms": [(rng.randrange(p), 0), (rng.randrange(p), 2)], "points": [rng.randrange(p)]}
    got = run(curve, columns, [job, other], n)
    assert got[0] == reference(p, columns, job, n)
    assert got[1] == reference(p, columns, other, n)


def test_nothing_to_do(h2):
    """n_jobs = 0 and n = 0 are H2_OK and enqueue nothing"""
    columns = [[1] * 16]
    job = {"terms": [(1, 0)], "points": [3]}
    lay = Layout(columns, [job], 16)
    table, terms, nt, lm, nl, pm, npts = tables("bn254", lay, [job])
    assert L().h2_poly_lincomb_device(0, table, 0, terms, nt, lm.ctypes.data, nl, pm.ctypes.data, npts, 16, None) == H2_OK
    assert L().h2_poly_lincomb_device(0, None, 0, None, 0, None, 0, None, 0, 16, None) == H2_OK
    assert L().h2_poly_lincomb_device(0, table, 1, terms, nt, lm.ctypes.data, nl, pm.ctypes.data, npts, 0, None) == H2_OK
    assert np.array_equal(lay.after(), lay.before)


def _rejected(curve_id, cols, js, rows, edit=None, **over):
    """the call with one thing wrong (an edit of the tables, or an argument given in `over`) is H2_EINVAL and writes nothing"""
    n = rows
    lay = Layout(cols, js, n)
    table, terms, nt, lm, nl, pm, npts = tables("bn254", lay, js)
    args = {"jobs": table, "n_jobs": len(js), "terms": terms, "n_terms": nt, "low": lm.ctypes.data, "n_low": nl,
            "points": pm.ctypes.data, "n_points": npts, "n": n}
    if edit:
        edit(table, terms, lay)
    args.update(over)
    st = L().h2_poly_lincomb_device(curve_id, args["jobs"], args["n_jobs"], args["terms"], args["n_terms"], args["low"],
                                    args["n_low"], args["points"], args["n_points"], args["n"], None)
    assert st == H2_EINVAL
    assert np.array_equal(lay.after(), lay.before)


def test_invalid_arguments(h2):
    n = 64
    columns = [[5] * n, [7] * n]
    jobs = [{"terms": [(2, 0), (3, 1)], "low": [1, 2], "points": [9]},
            {"terms": [(4, 1)], "low": [], "points": []}]
    _rejected(7, columns, jobs, n)                                                     # an unknown curve
    _rejected(0, columns, jobs, n, n=(1 << 30) + 1)                                    # n > 2^30
    _rejected(0, columns, jobs, n, n_terms=2)                                          # ranges past the arrays
    _rejected(0, columns, jobs, n, n_low=1)
    _rejected(0, columns, jobs, n, n_points=0)
    _rejected(0, columns, jobs, 1)                                                     # n_low = 2 > n = 1

    def too_many_rounds(table, terms, lay):
        table[0].n_points = max_rounds() + 1
    many = [dict(jobs[0], points=[9] * (max_rounds() + 1)), jobs[1]]
    _rejected(0, columns, many, n)
    _rejected(0, columns, jobs, n, edit=too_many_rounds, n_points=1 << 20)

    def null_out(table, terms, lay):
        table[1].d_out = None

    def odd_out(table, terms, lay):
        table[1].d_out = table[1].d_out + 8

    def null_poly(table, terms, lay):
        terms[2].d_poly = None

    def odd_poly(table, terms, lay):
        terms[0].d_poly = terms[0].d_poly + 8
    for edit in (null_out, odd_out, null_poly, odd_poly):
        _rejected(0, columns, jobs, n, edit=edit)
    _rejected(0, columns, jobs, n, jobs=None)                                          # null host arrays in use
    _rejected(0, columns, jobs, n, terms=None)
    _rejected(0, columns, jobs, n, low=None)
    _rejected(0, columns, jobs, n, points=None)

    # the overlaps
    def out_on_own_source(table, terms, lay):            # a dividing job may not write a source, its own included
        table[0].d_out = terms[0].d_poly

    def out_on_others_source(table, terms, lay):         # n_points = 0, but column 0 is job 0's source, not job 1's
        table[1].d_out = terms[0].d_poly

    def out_into_own_source(table, terms, lay):          # n_points = 0: an exact alias is fine, a shifted one is not
        table[1].d_out = terms[2].d_poly + 32

    def outs_overlap(table, terms, lay):
        table[1].d_out = table[0].d_out + 32 * (n - 1)

    def outs_equal(table, terms, lay):
        table[1].d_out = table[0].d_out
    for edit in (out_on_own_source, out_on_others_source, out_into_own_source, outs_overlap, outs_equal):
        _rejected(0, columns, jobs, n, edit=edit)
