"""The multiopen argument's column work over device-resident columns (include/h2hip.h: h2_poly_lincomb_device).

Upstream (halo2_proofs @6b43b6b, src/poly/kzg/multiopen/gwc/prover.rs and shplonk/prover.rs): both
provers build linear combinations of the opened polynomials, subtract a remainder of degree below the size of the rotation
set and divide out one to three linear factors.  `poly_lincomb` is the thin wrapper of the call; `gwc_open`,
`shplonk_open_h` and `shplonk_open_final` spell the two schemes' columns as its jobs, ONE call each.  The transcript stays
the caller's: the challenges come in as canonical ints, the columns go out for the caller to commit.
"""
import ctypes

import numpy as np

from . import lib as _lib


class LincombTerm(ctypes.Structure):
    """h2_lincomb_term_t"""
    _fields_ = [("d_poly", ctypes.c_void_p), ("coeff", ctypes.c_uint64 * 4)]


class LincombJob(ctypes.Structure):
    """h2_lincomb_job_t"""
    _fields_ = [("d_out", ctypes.c_void_p), ("first_term", ctypes.c_uint32), ("n_terms", ctypes.c_uint32),
                ("first_low", ctypes.c_uint32), ("n_low", ctypes.c_uint32), ("first_point", ctypes.c_uint32),
                ("n_points", ctypes.c_uint32)]


def max_rounds():
    """the largest number of points one job may divide out (host only)"""
    return _lib.load().h2_poly_lincomb_max_rounds()


def _column(t, n):
    if t.dtype.__str__() != "torch.int64" or not t.is_cuda or not t.is_contiguous() or t.dim() != 2 or t.shape[1] != 4:
        raise ValueError("columns must be contiguous (rows, 4) int64 CUDA tensors")
    if t.shape[0] < n:
        raise ValueError("a column of %d rows cannot hold %d" % (t.shape[0], n))
    return t.data_ptr()


def poly_lincomb(domain, jobs, n, stream=None):
    """ONE h2_poly_lincomb_device call.  jobs: (out, terms, low, points) each -- out a (>= n, 4) column or None for a new
    one; terms a list of (coefficient, column); low the canonical ints subtracted from the first len(low) rows; points the
    canonical ints z whose factors (X - z) are divided out in order, kate_division's way (the remainder dropped).
    -> the list of output columns: out[i] = sum_t coeff_t col_t[i] - low[i], then divided, over the first n rows."""
    import torch
    jobs = list(jobs)
    table = (LincombJob * max(1, len(jobs)))()
    n_terms = sum(len(j[1]) for j in jobs)
    terms = (LincombTerm * max(1, n_terms))()
    low, points, outs = [], [], []
    at = 0
    for i, (out, tms, lo, pts) in enumerate(jobs):
        if out is None:
            dev = tms[0][1].device if tms else "cuda"
            out = torch.empty((n, 4), dtype=torch.int64, device=dev)
        outs.append(out)
        J = table[i]
        J.d_out = _column(out, n)
        J.first_term, J.n_terms = at, len(tms)
        for c, col in tms:
            terms[at].d_poly = _column(col, n)
            terms[at].coeff[:] = [int(x) for x in domain.mont(c)]
            at += 1
        J.first_low, J.n_low = len(low), len(lo)
        low.extend(lo)
        J.first_point, J.n_points = len(points), len(pts)
        points.extend(pts)
    lm = np.concatenate([domain.mont(x) for x in low]) if low else None
    pm = np.concatenate([domain.mont(x) for x in points]) if points else None
    st = domain._L.h2_poly_lincomb_device(domain.curve, table, len(jobs), terms, n_terms,
                                          lm.ctypes.data if low else None, len(low),
                                          pm.ctypes.data if points else None, len(points), n,
                                          ctypes.c_void_p(stream) if stream is not None else domain._stream())
    _lib.check(st, "h2_poly_lincomb_device")
    return outs


def interpolate(p, points, values):
    """coefficients of the polynomial of degree < len(points) through (points[i], values[i]) over the field of p elements"""
    out = [0] * len(points)
    for i, (xi, yi) in enumerate(zip(points, values)):
        term, den = [1], 1
        for j, xj in enumerate(points):
            if j != i:
                nt = [0] * (len(term) + 1)
                for d, c in enumerate(term):
                    nt[d] = (nt[d] - c * xj) % p
                    nt[d + 1] = (nt[d + 1] + c) % p
                term = nt
                den = den * (xi - xj) % p
        scale = yi * pow(den, -1, p) % p
        for d, c in enumerate(term):
            out[d] = (out[d] + c * scale) % p
    return out


def _horner(p, coeffs, x):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % p
    return acc


def gwc_open(domain, queries, v):
    """ProverGWC::create_proof's witness polynomials.  queries: (point, column, ...) in the prover's order; v: the
    challenge.  -> a (points, n, 4) tensor, one witness per distinct point in first-appearance order:
    kate_division(sum_k v^k poly_k, point) over the queries at that point.  One h2_poly_lincomb_device call."""
    import torch
    p = domain.p
    points = []
    for q in queries:
        if q[0] not in points:
            points.append(q[0])
    if not points:
        return torch.empty((0, 0, 4), dtype=torch.int64, device="cuda")
    n = queries[0][1].shape[0]
    out = torch.empty((len(points), n, 4), dtype=torch.int64, device=queries[0][1].device)
    jobs = []
    for i, pt in enumerate(points):
        terms, vp = [], 1
        for q in queries:
            if q[0] == pt:
                terms.append((vp, q[1]))
                vp = vp * v % p
        jobs.append((out[i], terms, [], [pt]))
    poly_lincomb(domain, jobs, n)
    return out


def rotation_sets(queries):
    """ProverSHPLONK's grouping: -> [(sorted point set, [(key, column)])], sets and members in first-appearance order.
    queries: (point, column, key); a polynomial is known by its key."""
    polys = []
    for pt, col, key in queries:
        for entry in polys:
            if entry[0] == key:
                if pt not in entry[2]:
                    entry[2].append(pt)
                break
        else:
            polys.append((key, col, [pt]))
    groups = []
    for key, col, pts in polys:
        pset = sorted(pts)
        for g in groups:
            if g[0] == pset:
                g[1].append((key, col))
                break
        else:
            groups.append((pset, [(key, col)]))
    return groups


def shplonk_open_h(domain, queries, evals, y, v):
    """ProverSHPLONK::create_proof up to h(X) = sum_i v^i (sum_j y^j (p_ij - r_ij)) / Z_i.  queries: (point, column, key);
    evals[(key, point)]: the evaluations, canonical ints; y, v: the challenges.  -> (h, state): the column to commit and
    what shplonk_open_final needs.  One h2_poly_lincomb_device call: a job per rotation set with v^i folded into its
    coefficients and remainder, the sets' quotients then added into the first (a job's output cannot feed another job)."""
    p = domain.p
    groups = rotation_sets(queries)
    n = queries[0][1].shape[0]
    if max(len(g[0]) for g in groups) > max_rounds():
        raise ValueError("a rotation set has more points than one job divides out")
    jobs, per_set, vp = [], [], 1
    for pset, members in groups:
        terms, rsum, rems, yp = [], [0] * len(pset), [], 1
        for key, col in members:
            r = interpolate(p, pset, [evals[(key, pt)] for pt in pset])
            rems.append(r)
            terms.append((vp * yp % p, col))
            rsum = [(a + vp * yp % p * b) % p for a, b in zip(rsum, r)]
            yp = yp * y % p
        jobs.append((None, terms, rsum, pset))
        per_set.append((pset, members, rems))
        vp = vp * v % p
    outs = poly_lincomb(domain, jobs, n)
    h = outs[0]
    for q in outs[1:]:
        domain.pointwise("add", h, q)
    state = {"domain": domain, "n": n, "sets": per_set, "y": y, "v": v, "h": h,
             "points": sorted({pt for pset, _ in groups for pt in pset})}
    return h, state


def shplonk_open_final(state, u):
    """ProverSHPLONK::create_proof's last quotient: (L(X) / (X - u)) / Z_{T \\ S_0}(u) with
    L = sum_i v^i Z_{T \\ S_i}(u) sum_j y^j (p_ij - r_ij(u)) - Z_T(u) h.  One h2_poly_lincomb_device call; the 1 / z_0
    scale rides in the coefficients."""
    domain, y, v = state["domain"], state["y"], state["v"]
    p, T = domain.p, state["points"]
    zt = 1
    for pt in T:
        zt = zt * (u - pt) % p
    z_of = []
    for pset, _, _ in state["sets"]:
        z_i = 1
        for pt in T:
            if pt not in pset:
                z_i = z_i * (u - pt) % p
        z_of.append(z_i)
    z0_inv = pow(z_of[0], -1, p)
    terms, const, vp = [], 0, 1
    for (pset, members, rems), z_i in zip(state["sets"], z_of):
        w, yp = vp * z_i % p * z0_inv % p, 1
        for (key, col), r in zip(members, rems):
            terms.append((w * yp % p, col))
            const = (const + w * yp % p * _horner(p, r, u)) % p
            yp = yp * y % p
        vp = vp * v % p
    terms.append(((p - zt) * z0_inv % p, state["h"]))
    return poly_lincomb(domain, [(None, terms, [const], [u])], state["n"])[0]
