"""The inner product argument over a registered SRS table (include/h2hip.h: h2_ipa_*).

Upstream (halo2_proofs, src/poly/ipa/commitment.rs and commitment/{prover,verifier}.rs -- un-vendored; the algorithm is
restated in DESIGN.md section 7.13): the opening proof a halo2 host on the Pasta curves ends `create_proof` with.
`ParamsIPA` registers the bases ONCE as g || u || w; `create_proof` runs the k rounds on that table -- no generator is
ever folded, each round is one two-column MSM over the registered table -- and `verify_proof` checks
    sum [u_j^-1] L_j + P' + sum [u_j] R_j == [c] <s, G> + [c b_0 z] U + [f] W,   P' = P - [v] G[0] + [xi] S
with <s, G> and the U, W, G[0] terms as ONE h2_msm_device on the same table (s from h2_ipa_challenge_products_device).
`create_proofs` runs m openings in lockstep through h2_ipa_*_batch_device -- a round of all of them is ONE MSM of 2 m columns
on the table; it is the one prover path, `create_proof` is its batch of one (the C ABI's single
calls h2_ipa_begin_device / h2_ipa_round_device / h2_ipa_final_device are the batch calls at m = 1 too).
`verify_proofs` checks N such proofs behind ONE combined equation: the N equations are linear in the same table, so with
random weights r_p they collapse into one table MSM and one points MSM; the 2k + 1 compressed
points of every proof are decompressed by one kernel launch (h2_pasta_points_decompress_device) and the weighted sum of the
N compute_s vectors comes from h2_ipa_challenge_products_sum_device, none of them materialised.
`verify_proofs_bytes` is the same verifier behind ONE C ABI call, h2_ipa_verify_proofs: the transcripts are replayed on the
device from exported Blake2b midstates and the scalars of every combined check are made there.
`create_proofs_bytes` is the prover behind ONE C ABI call, h2_ipa_create_proofs: the transcripts run on the device too, a
lane per opening behind every round's MSM, so no round reads anything back.
Polynomials are (n, 4) int64 CUDA tensors viewing 4 x u64 Montgomery limbs (numpy uint64 arrays are uploaded); points are
affine (x, y) pairs of canonical ints, None for the identity.  The transcript is transcript.Blake2bTranscript on the
curve.  `ParamsIPA::new`'s hash-to-curve is not here: the bases are the caller's.  There is no CPU fallback.
"""
import ctypes
import os

import numpy as np

from . import lib as _lib
from .api import Bases, _as_u64, _curve_id, _ensure_init, msm_points, msm_points_device
from .domain import EvaluationDomain
from .opening import poly_lincomb
from .transcript import FIELDS, Blake2bTranscript  # noqa: F401


def compute_s(u, init, p):
    """upstream's compute_s: s[i] = init * prod over the set bits t of i of u[k-1-t] (mod p), 2^k entries"""
    s = [init % p]
    for uj in u:                                    # s^(j+1)[2h] = s^(j)[h], s^(j+1)[2h+1] = s^(j)[h] u_j
        s = [v for x in s for v in (x, x * uj % p)]
    return s


def compute_b(x, u, p):
    """upstream's compute_b: prod_t (1 + u[k-1-t] x^(2^t)) = <compute_s(u, 1), powers of x> (mod p)"""
    out, cur = 1, x % p
    for uj in reversed(u):
        out = out * (1 + uj * cur) % p
        cur = cur * cur % p
    return out


def _limbs(v):
    return np.array([(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)


def _ints(raw):
    raw = bytes(raw)
    return [int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)]


def random_scalar(rng, p):
    """ff's Field::random: 64 bytes of the rng as a little-endian integer, reduced"""
    return int.from_bytes(bytes(rng(64)), "little") % p


class ParamsIPA:
    """ParamsIPA<C> for the prover and the verifier: g (n affine points), w, u, registered as g || u || w."""

    def __init__(self, curve, k, g, w, u):
        _ensure_init()
        self.curve = _curve_id(curve)
        self.k, self.n = int(k), 1 << int(k)
        self.p, self.q, _ = FIELDS[self.curve]
        self.R, self.Rq = (1 << 256) % self.p, (1 << 256) % self.q
        self.Rq_inv = pow(self.Rq, -1, self.q)
        g = _as_u64(g, 8, "g")
        if g.shape[0] != self.n:
            raise ValueError("ParamsIPA: g.len() != 1 << k")
        self.g = g
        self.w = _as_u64(w, 8, "w").reshape(1, 8)
        self.u = _as_u64(u, 8, "u").reshape(1, 8)
        self.bases = Bases(self.curve, np.concatenate([g, self.u, self.w]))
        self.domain = EvaluationDomain(2, self.k, self.curve)
        self._L = _lib.load()

    # ---- helpers --------------------------------------------------------------------------------------------
    def mont(self, v):
        return _limbs(v % self.p * self.R % self.p)

    def column(self, poly):
        """a polynomial as a (rows, 4) int64 CUDA tensor"""
        import torch
        if isinstance(poly, torch.Tensor):
            return poly
        return torch.from_numpy(_as_u64(poly, 4, "poly").view(np.int64).copy()).cuda()

    def affine_ints(self, limbs):
        """8 Montgomery limbs of an affine point -> (x, y) canonical ints, None for (0, 0)"""
        x, y = _ints(np.ascontiguousarray(limbs, dtype=np.uint64).tobytes())
        if x == 0 and y == 0:
            return None
        return (x * self.Rq_inv % self.q, y * self.Rq_inv % self.q)

    def affine_limbs(self, pt):
        x, y = pt if pt is not None else (0, 0)
        return np.concatenate([_limbs(x * self.Rq % self.q), _limbs(y * self.Rq % self.q)])

    def jac_to_affine(self, jac):
        """12 Montgomery limbs (X, Y, Z), x = X / Z^2, y = Y / Z^3 -> (x, y) canonical ints or None"""
        X, Y, Z = [v * self.Rq_inv % self.q for v in _ints(np.ascontiguousarray(jac, dtype=np.uint64).tobytes())]
        if Z == 0:
            return None
        zi = pow(Z, -1, self.q)
        return (X * zi * zi % self.q, Y * zi * zi % self.q * zi % self.q)

    def msm_table(self, d_col):
        """ONE h2_msm_device over g || u || w: d_col a (n + 2, 4) column -> affine ints"""
        import torch
        out = torch.empty(12, dtype=torch.int64, device=d_col.device)
        self.bases.msm_device(d_col.data_ptr(), self.n + 2, 1, out.data_ptr(), self.domain._stream().value or 0)
        return self.jac_to_affine(out.cpu().numpy().view(np.uint64))

    def commit(self, poly, blind):
        """commit(poly, r) = <poly, g> + [r] w: h2_msm_device on the column poly || 0 || r"""
        import torch
        poly = self.column(poly)
        if poly.shape[0] != self.n:
            raise ValueError("commit: poly.len() != n")
        tail = torch.from_numpy(np.stack([_limbs(0), self.mont(blind)]).view(np.int64)).to(poly.device)
        return self.msm_table(torch.cat([poly, tail]))


def create_proof(params, transcript, p, p_blind, x3, rng, s_poly=None):
    """ipa::commitment::prover::create_proof: opens the polynomial p (n coefficients, committed with blind p_blind) at x3.
    rng: a callable n -> n bytes.  Written to the transcript: S, then k x (L_j, R_j), then c, then f.

    s_poly: the caller's column of n random coefficients, or None.  With None it is ONE 32-byte draw of the rng expanded on
    the device by h2_chacha20_scalars_device -- the one deviation from upstream's draw order, which takes the n scalars
    from the rng one by one.  Everything else is drawn in upstream's order: s_blind, then l_j and r_j of every round.
    Each round reads 128 bytes back (L_j || R_j) for the transcript; the final call reads 64.  A ValueError for a p or an
    s_poly that does not have n coefficients.  It is create_proofs' batch of one."""
    return create_proofs(params, [(transcript, p, p_blind, x3, rng, s_poly)])[0]


MAX_BATCH = 64                                      # H2_IPA_MAX_BATCH


def create_proofs(params, items):
    """create_proof for a batch, in lockstep: items = sequence of (transcript, p, p_blind, x3, rng, s_poly or None), all on
    the same params -> list[bytes], entry i exactly the bytes of create_proof(params, *items[i]), transcript i left where
    create_proof leaves it.  Every item has its OWN transcript and its OWN rng, drawn from in create_proof's order (the
    32-byte seed when s_poly is None, s_blind, then l_j and r_j of every round); one rng object shared between items is
    drawn from in another order than m create_proof calls would and breaks the equality.

    The m openings advance together (h2_ipa_*_batch_device): the 2 m values s_poly_i(x3_i), p_i(x3_i) are one
    h2_poly_eval_device call; the corrections of the constant terms and the m polynomials p' are h2_poly_lincomb_device
    calls of m jobs; the m commitments to S are ONE h2_msm_device of m columns of n + 2; a round is one call, one MSM of
    2 m columns and one read-back of m x 128 bytes; the final is one call and m x 64 bytes.  Calls and read-backs per batch:
    k + a constant, whatever m is -- but for the items with s_poly None, each expanded from its own seed by its own
    h2_chacha20_scalars_device call (no read-back).  More than H2_IPA_MAX_BATCH items go through in groups of that many."""
    items = list(items)
    out = []
    for first in range(0, len(items), MAX_BATCH):
        out.extend(_create_proofs_group(params, items[first:first + MAX_BATCH]))
    return out


def _create_proofs_group(params, items):
    import torch
    L, cv, k, n, P = params._L, params.curve, params.k, params.n, params.p
    dom = params.domain
    stream = dom._stream()
    m = len(items)
    trs = [it[0] for it in items]
    ps = [params.column(it[1]) for it in items]
    if any(p.shape[0] != n for p in ps):
        raise ValueError("create_proofs: p.len() != n")
    blinds, x3s, rngs = [it[2] for it in items], [it[3] for it in items], [it[4] for it in items]
    dev = ps[0].device
    rinv = pow(params.R, -1, P)

    def scalars(values):
        return np.concatenate([params.mont(v) for v in values])

    def upload(values):
        return torch.from_numpy(scalars(values).reshape(-1, 4).view(np.int64)).to(dev)

    # the m columns s_poly_i || 0 || s_blind_i the commitments are taken of
    cols = torch.zeros((m, n + 2, 4), dtype=torch.int64, device=dev)
    for i, it in enumerate(items):
        if it[5] is None:
            seed = bytes(rngs[i](32))
            _lib.check(L.h2_chacha20_scalars_device(cv, seed, 0, n, ctypes.c_void_p(cols[i].data_ptr()), stream),
                       "h2_chacha20_scalars_device")
        else:
            s_poly = params.column(it[5])
            if s_poly.shape[0] != n:
                raise ValueError("create_proofs: s_poly.len() != n")
            cols[i, :n] = s_poly
    # s_poly_i(x3_i) and p_i(x3_i): one call, one read-back
    ptrs = (ctypes.c_void_p * (2 * m))(*([cols[i].data_ptr() for i in range(m)] + [p.data_ptr() for p in ps]))
    vals = torch.empty((2 * m, 4), dtype=torch.int64, device=dev)
    x3m = scalars(x3s + x3s)                          # a local: the array must outlive the call that reads its address
    _lib.check(L.h2_poly_eval_device(cv, ptrs, n, x3m.ctypes.data, 2 * m, ctypes.c_void_p(vals.data_ptr()), stream),
               "h2_poly_eval_device")
    vals = [x * rinv % P for x in _ints(vals.cpu().numpy().tobytes())]
    s_at, v = vals[:m], vals[m:]
    # s_poly_i[0] -= s_poly_i(x3_i): the blinding polynomials have their roots
    poly_lincomb(dom, [(cols[i], [(1, cols[i])], [s_at[i]], []) for i in range(m)], n)
    s_blind = [random_scalar(rng, P) for rng in rngs]
    cols[:, n + 1] = upload(s_blind)
    jac = torch.empty((m, 12), dtype=torch.int64, device=dev)
    params.bases.msm_device(cols.data_ptr(), n + 2, m, jac.data_ptr(), stream.value or 0)
    jac = jac.cpu().numpy().view(np.uint64)
    xi, z = [], []
    for i, tr in enumerate(trs):
        tr.write_point(params.jac_to_affine(jac[i]))
        xi.append(tr.squeeze_challenge())
        z.append(tr.squeeze_challenge())
    # p'_i = s_poly_i xi_i + p_i, p'_i[0] -= p_i(x3_i)
    p_prime = poly_lincomb(dom, [(None, [(xi[i], cols[i]), (1, ps[i])], [v[i]], []) for i in range(m)], n)
    f = [(s_blind[i] * xi[i] + blinds[i]) % P for i in range(m)]

    need = ctypes.c_size_t(0)
    _lib.check(L.h2_ipa_batch_state_bytes(k, m, ctypes.byref(need)), "h2_ipa_batch_state_bytes")
    state = torch.empty(need.value // 8, dtype=torch.int64, device=dev)
    out = torch.empty((m, 16), dtype=torch.int64, device=dev)
    d_p = (ctypes.c_void_p * m)(*[t.data_ptr() for t in p_prime])
    _lib.check(L.h2_ipa_begin_batch_device(cv, k, m, d_p, x3m.ctypes.data, ctypes.c_void_p(state.data_ptr()), stream),   # its first m
               "h2_ipa_begin_batch_device")
    zm = scalars(z)
    u = u_inv = None
    for j in range(k):
        l_j, r_j = [], []
        for rng in rngs:
            l_j.append(random_scalar(rng, P))
            r_j.append(random_scalar(rng, P))
        um, uim = (scalars(u), scalars(u_inv)) if j else (None, None)
        lm, rm = scalars(l_j), scalars(r_j)
        st = L.h2_ipa_round_batch_device(cv, params.bases.handle, k, j, m, ctypes.c_void_p(state.data_ptr()),
                                         um.ctypes.data if j else None, uim.ctypes.data if j else None, zm.ctypes.data,
                                         lm.ctypes.data, rm.ctypes.data, ctypes.c_void_p(out.data_ptr()), stream)
        _lib.check(st, "h2_ipa_round_batch_device")
        lr = out.cpu().numpy().view(np.uint64)
        u, u_inv = [], []
        for i, tr in enumerate(trs):
            tr.write_point(params.affine_ints(lr[i, :8]))
            tr.write_point(params.affine_ints(lr[i, 8:]))
            u.append(tr.squeeze_challenge())
            u_inv.append(pow(u[i], -1, P))
            f[i] = (f[i] + l_j[i] * u_inv[i] + r_j[i] * u[i]) % P
    um, uim = scalars(u), scalars(u_inv)
    _lib.check(L.h2_ipa_final_batch_device(cv, k, m, ctypes.c_void_p(state.data_ptr()), um.ctypes.data, uim.ctypes.data,
                                           ctypes.c_void_p(out.data_ptr()), stream), "h2_ipa_final_batch_device")
    cb = out.reshape(-1)[:8 * m].cpu().numpy().reshape(m, 8)
    proofs = []
    for i, tr in enumerate(trs):
        tr.write_scalar(_ints(cb[i, :4].tobytes())[0] * rinv % P)
        tr.write_scalar(f[i])
        proofs.append(bytes(tr.bytes))
    return proofs


def create_proofs_bytes(params, items):
    """create_proofs through ONE C ABI call per group of MAX_BATCH (h2_ipa_create_proofs): items as
    create_proofs takes them, (transcript, p, p_blind, x3, rng, s_poly or None), each transcript a transcript.Blake2bMidstate
    standing where create_proof would start -> list[bytes], entry i the (2k + 3) * 32 bytes create_proof writes for the item;
    midstate i is advanced to where create_proof leaves the transcript (behind f).  The transcripts run on the device, one
    lane per opening: from round 0 to f nothing goes through the host.

    Every random value is drawn up front from the item's own rng in create_proof's order -- the 32-byte seed when s_poly is
    None, s_blind, then l_j, r_j for j = 0 .. k - 1; none depends on the transcript, so the stream per item is the one
    create_proofs draws.  A ValueError for BN254 (the wire form is the Pasta one) and for a p or an s_poly that does not have
    n coefficients; a RuntimeError if a challenge came out zero (probability about 2^-254 per round)."""
    if params.curve == 0:
        raise ValueError("create_proofs_bytes: the Pasta wire form; BN254 openings go through create_proofs")
    items = list(items)
    out = []
    for first in range(0, len(items), MAX_BATCH):
        out.extend(_create_proofs_bytes_group(params, items[first:first + MAX_BATCH]))
    return out


def _create_proofs_bytes_group(params, items):
    from .transcript import STATE_BYTES
    k, n, P, m = params.k, params.n, params.p, len(items)
    ps = [params.column(it[1]) for it in items]
    if any(p.shape[0] != n for p in ps):
        raise ValueError("create_proofs_bytes: p.len() != n")
    s_polys = [None if it[5] is None else params.column(it[5]) for it in items]
    if any(s is not None and s.shape[0] != n for s in s_polys):
        raise ValueError("create_proofs_bytes: s_poly.len() != n")
    seeds = bytearray(32 * m)
    s_blind, round_blinds = [], []
    for i, it in enumerate(items):
        rng = it[4]
        if s_polys[i] is None:
            seeds[32 * i:32 * i + 32] = bytes(rng(32))
        s_blind.append(random_scalar(rng, P))
        round_blinds.extend(random_scalar(rng, P) for _ in range(2 * k))

    def scalars(values):
        return np.ascontiguousarray(np.concatenate([params.mont(v) for v in values]))

    states = bytearray()
    for it in items:
        st = it[0].export()
        if len(st) != STATE_BYTES:
            raise ValueError("create_proofs_bytes: a midstate is %d bytes" % STATE_BYTES)
        states += st
    states = (ctypes.c_char * len(states)).from_buffer(states)
    seeds = (ctypes.c_char * len(seeds)).from_buffer(seeds)
    d_p = (ctypes.c_void_p * m)(*[p.data_ptr() for p in ps])
    d_s = (ctypes.c_void_p * m)(*[None if s is None else s.data_ptr() for s in s_polys])
    pb, x3, sb, rb = scalars([it[2] for it in items]), scalars([it[3] for it in items]), scalars(s_blind), scalars(round_blinds)
    per = (2 * k + 3) * 32
    proofs = ctypes.create_string_buffer(m * per)
    states_out = ctypes.create_string_buffer(m * STATE_BYTES)
    status = (ctypes.c_uint32 * m)()
    st = params._L.h2_ipa_create_proofs(params.curve, params.bases.handle, k, m, states, d_p, pb.ctypes.data, x3.ctypes.data, d_s, seeds,
                                        sb.ctypes.data, rb.ctypes.data, proofs, states_out, status)
    _lib.check(st, "h2_ipa_create_proofs")
    if any(status):
        raise RuntimeError("create_proofs_bytes: a challenge of opening %d was zero" % list(status).index(1))
    for i, it in enumerate(items):
        it[0]._st.raw = states_out.raw[i * STATE_BYTES:(i + 1) * STATE_BYTES]
    return [proofs.raw[i * per:(i + 1) * per] for i in range(m)]


def verify_proof(params, transcript, P, x3, v):
    """ipa::commitment::verifier::verify_proof on a reading transcript: does the proof open the commitment P (affine ints)
    to v at x3?  <s, G> and the G[0], U, W terms are one h2_msm_device on the registered table, s from
    h2_ipa_challenge_products_device; P, S and the 2k points L_j, R_j go through h2_msm_points.  -> bool"""
    import torch
    from .transcript import TranscriptError
    L, cv, k, n, p = params._L, params.curve, params.k, params.n, params.p
    dom = params.domain
    try:
        S = transcript.read_point()
        xi = transcript.squeeze_challenge()
        z = transcript.squeeze_challenge()
        rounds = []
        for _ in range(k):
            l_pt = transcript.read_point()
            r_pt = transcript.read_point()
            rounds.append((l_pt, r_pt, transcript.squeeze_challenge()))
        c = transcript.read_scalar()
        f = transcript.read_scalar()
    except TranscriptError:
        return False
    u = [r[2] for r in rounds]
    if any(x == 0 for x in u):
        return False
    b0 = compute_b(x3, u, p)
    # everything on one side: sum [1/u_j] L_j + P + [xi] S + sum [u_j] R_j - [v] G[0] - [c] <s, G> - [c b0 z] U - [f] W == 0
    um = np.concatenate([params.mont(x) for x in u])
    col = torch.empty((n + 2, 4), dtype=torch.int64, device="cuda")
    st = L.h2_ipa_challenge_products_device(cv, um.ctypes.data, k, params.mont(-c).ctypes.data, ctypes.c_void_p(col.data_ptr()),
                                            dom._stream())
    _lib.check(st, "h2_ipa_challenge_products_device")
    poly_lincomb(dom, [(col, [(1, col)], [v % p], [])], n)                                 # col[0] -= v
    tail = np.stack([params.mont(-c * b0 % p * z), params.mont(-f)])
    col[n:] = torch.from_numpy(tail.view(np.int64)).to(col.device)
    table_side = params.msm_table(col)
    terms = [(1, P), (xi, S)]
    for l_pt, r_pt, uj in rounds:
        terms.append((pow(uj, -1, p), l_pt))
        terms.append((uj, r_pt))
    terms = [(s, pt) for s, pt in terms if pt is not None]
    if terms:
        other = params.jac_to_affine(msm_points(np.stack([params.mont(s) for s, _ in terms]),
                                                np.stack([params.affine_limbs(pt) for _, pt in terms]), cv))
    else:
        other = None
    if table_side is None or other is None:
        return table_side is None and other is None
    return table_side[0] == other[0] and (table_side[1] + other[1]) % params.q == 0


def challenge_products_sum(curve, k, u, init, out=None):
    """sum_p compute_s(u[p], init[p]) as a (2^k, 4) int64 CUDA tensor (h2_ipa_challenge_products_sum_device), over the scalar
    field of `curve`, on the current stream: u a list of `count` challenge lists (k canonical ints each), init `count`
    canonical ints.  out: a CUDA tensor to write into (its first 2^k rows), or None."""
    import torch
    from .poseidon import _stream
    _ensure_init()
    cv = _curve_id(curve)
    p = FIELDS[cv][0]
    R = (1 << 256) % p
    count = len(u)
    if len(init) != count or any(len(x) != k for x in u):
        raise ValueError("challenge_products_sum: count x k challenges and count inits")
    um = np.concatenate([_limbs(x % p * R % p) for row in u for x in row]) if count else None
    im = np.concatenate([_limbs(x % p * R % p) for x in init]) if count else None
    if out is None:
        out = torch.empty((1 << k, 4), dtype=torch.int64, device="cuda")
    st = _lib.load().h2_ipa_challenge_products_sum_device(cv, um.ctypes.data if count else None, im.ctypes.data if count else None,
                                                          k, count, ctypes.c_void_p(out.data_ptr()), _stream())
    _lib.check(st, "h2_ipa_challenge_products_sum_device")
    return out


class _Replayed:
    """what the replay of one transcript leaves for the combined check"""
    __slots__ = ("first", "P", "v", "xi", "z", "u", "u_inv", "c", "f", "b0")


def verify_proofs(params, items, rng=None, stats=None):
    """verify_proof for a batch: items = sequence of (reading transcript, P, x3, v), each transcript positioned where
    verify_proof would start -> list[bool], entry i exactly what verify_proof(params, *items[i]) returns, every transcript
    left where verify_proof leaves it.  rng: a callable n -> n bytes (default os.urandom) for the weights, 16 bytes per proof,
    little-endian, a zero weight redrawn.  stats: an optional dict, filled with {"checks": combined checks run, "points":
    points decompressed, "rejected_early": items refused before any check}.

    One decompression launch and one read-back for all the points; the host replays the transcripts with the decoded points
    (no square root on the host); then ONE combined check -- the challenge-product sum, one h2_msm_device on the registered
    table, one h2_msm_points_device whose point operand is the decompression's own output with the commitments uploaded
    behind it -- and 96 bytes read back.  A failing batch is halved on the replayed data until every culprit is alone."""
    import torch
    from .transcript import TranscriptError
    if params.curve == 0:
        raise ValueError("verify_proofs: the Pasta wire form; BN254 proofs go through verify_proof")
    rng = rng or os.urandom
    items = list(items)
    N = len(items)
    st = {"checks": 0, "points": 0, "rejected_early": 0}
    if stats is not None:
        stats.update(st)
    if N == 0:
        return []
    L, cv, k, n, p, q = params._L, params.curve, params.k, params.n, params.p, params.q
    dom = params.domain
    stream = dom._stream()
    per = 2 * k + 1
    # 1. gather: the compressed points that are there, item after item
    chunks, first = [], []
    for tr, _, _, _ in items:
        have = 0 if tr.buf is None else max(0, min(per, (len(tr.buf) - tr.pos) // 32))
        first.append(len(chunks))
        chunks.extend(tr.buf[tr.pos + 32 * j:tr.pos + 32 * j + 32] for j in range(have))
    first.append(len(chunks))
    G = len(chunks)
    st["points"] = G
    # 2. decompress: one launch, one read-back.  The affine output is the front of the points MSM's operand
    d_points = torch.zeros((G + N, 8), dtype=torch.int64, device="cuda")
    status = b""
    aff = np.zeros((0, 8), dtype=np.uint64)
    if G:
        d_wire = torch.from_numpy(np.frombuffer(b"".join(chunks), dtype=np.int64).copy()).cuda()
        d_status = torch.empty(G, dtype=torch.uint8, device="cuda")
        _lib.check(L.h2_pasta_points_decompress_device(cv, ctypes.c_void_p(d_wire.data_ptr()), G, ctypes.c_void_p(d_points.data_ptr()),
                                                       ctypes.c_void_p(d_status.data_ptr()), stream), "h2_pasta_points_decompress_device")
        back = torch.cat([d_points[:G].reshape(-1).view(torch.uint8), d_status]).cpu().numpy()
        aff, status = back[:64 * G].view(np.uint64).reshape(G, 8), bytes(back[64 * G:])
    # 3. replay on the host with the decoded points
    ok = [False] * N
    live = {}
    for i, (tr, P, x3, v) in enumerate(items):
        lo, hi = first[i], first[i + 1]
        cursor = [lo]

        def point():
            j = cursor[0]
            cursor[0] += 1
            if j >= hi:
                return tr.read_point()                       # no bytes left: raises as verify_proof's read would
            return tr.read_point_decoded(params.affine_ints(aff[j]) if status[j] == 0 else None, status[j])
        try:
            point()
            xi = tr.squeeze_challenge()
            z = tr.squeeze_challenge()
            u = []
            for _ in range(k):
                point()
                point()
                u.append(tr.squeeze_challenge())
            c = tr.read_scalar()
            f = tr.read_scalar()
        except TranscriptError:
            st["rejected_early"] += 1
            continue
        if any(x == 0 for x in u):
            st["rejected_early"] += 1
            continue
        r = _Replayed()
        r.first, r.P, r.v, r.xi, r.z, r.u, r.c, r.f = lo, P, v % p, xi, z, u, c, f
        r.u_inv = [pow(x, -1, p) for x in u]
        r.b0 = compute_b(x3, u, p)
        live[i] = r
    if live:
        d_points[G:] = torch.from_numpy(np.stack([params.affine_limbs(P) for _, P, _, _ in items]).view(np.int64)).cuda()
    col = torch.empty((n + 2, 4), dtype=torch.int64, device="cuda")
    jac = torch.empty(24, dtype=torch.int64, device="cuda")
    total = torch.empty(12, dtype=torch.int64, device="cuda")

    def weight():
        while True:
            w = int.from_bytes(bytes(rng(16)), "little")
            if w:
                return w

    def check(subset):
        """sum_p r_p (sum [1/u_j] L_j + P + [xi] S + sum [u_j] R_j - [v] G[0] - [c] <s, G> - [c b0 z] U - [f] W) == 0 over the subset"""
        st["checks"] += 1
        scal = np.zeros((G + N, 4), dtype=np.uint64)
        inits, row0, tail_u, tail_w = [], 0, 0, 0
        for i in subset:
            r, w = live[i], weight()
            inits.append(-w * r.c % p)
            row0 += w * r.v
            tail_u += w * r.c % p * r.b0 % p * r.z
            tail_w += w * r.f
            scal[r.first] = params.mont(w * r.xi)
            for j in range(k):
                scal[r.first + 1 + 2 * j] = params.mont(w * r.u_inv[j])
                scal[r.first + 2 + 2 * j] = params.mont(w * r.u[j])
            if r.P is not None:
                scal[G + i] = params.mont(w)
        challenge_products_sum(cv, k, [live[i].u for i in subset], inits, out=col)
        poly_lincomb(dom, [(col, [(1, col)], [row0 % p], [])], n)                        # col[0] -= sum r_p v_p
        col[n:] = torch.from_numpy(np.stack([params.mont(-tail_u), params.mont(-tail_w)]).view(np.int64)).to(col.device)
        d_scal = torch.from_numpy(scal.view(np.int64)).cuda()
        params.bases.msm_device(col.data_ptr(), n + 2, 1, jac.data_ptr(), stream.value or 0)
        msm_points_device(d_points.data_ptr(), d_scal.data_ptr(), G + N, G + N, 1, jac.data_ptr() + 96, stream.value or 0, cv)
        params.bases.points_sum_device(jac.data_ptr(), 2, 1, total.data_ptr(), stream.value or 0)
        Z = total[8:].cpu().numpy()
        return not Z.any()

    def settle(subset, known_bad):
        """the verdicts of a subset; known_bad: a combined check has already shown that it holds a culprit"""
        if not known_bad and check(subset):
            for i in subset:
                ok[i] = True
            return
        if len(subset) == 1:
            return                                            # a singleton's verdict is its own equation; r != 0
        half = len(subset) // 2
        left, right = subset[:half], subset[half:]
        if check(left):
            for i in left:
                ok[i] = True
            settle(right, len(right) > 1)                     # the culprits are on the other side; one alone is still checked
        else:
            settle(left, True)
            settle(right, False)

    if live:
        settle(sorted(live), False)
    if stats is not None:
        stats.update(st)
    return ok


def verify_proofs_bytes(params, items, rng=None, stats=None):
    """verify_proofs through ONE C ABI call (h2_ipa_verify_proofs): items = sequence of (midstate,
    proof, P, x3, v) -- the midstate the 208 bytes of a transcript.Blake2bMidstate export (or the object) standing where
    verify_proof would start, the proof exactly its (2k + 3) * 32 bytes -- -> list[bool], entry i what verify_proof gives for
    the item.  The transcripts are replayed on the device, one lane per proof, and the scalars of every combined check are
    made there: nothing but the weights comes from the host between the upload and a check's 96 bytes.  rng: a callable
    n -> n bytes (default: the OS) for the weights, drawn as verify_proofs draws them.  stats: an optional dict, filled with
    {"checks": combined checks run}."""
    if params.curve == 0:
        raise ValueError("verify_proofs_bytes: the Pasta wire form; BN254 proofs go through verify_proof")
    items = list(items)
    N = len(items)
    if stats is not None:
        stats.update({"checks": 0})
    if N == 0:
        return []
    from .transcript import STATE_BYTES
    states = bytearray()
    for it in items:
        st = it[0].export() if hasattr(it[0], "export") else bytes(it[0])
        if len(st) != STATE_BYTES:
            raise ValueError("verify_proofs_bytes: a midstate is %d bytes" % STATE_BYTES)
        states += st
    states = (ctypes.c_char * len(states)).from_buffer(states)
    bufs = [bytes(it[1]) for it in items]
    ptrs = (ctypes.c_char_p * N)(*bufs)
    lens = (ctypes.c_size_t * N)(*[len(b) for b in bufs])
    commitments = np.ascontiguousarray(np.stack([params.affine_limbs(it[2]) for it in items]))
    x3 = np.ascontiguousarray(np.stack([params.mont(it[3]) for it in items]))
    v = np.ascontiguousarray(np.stack([params.mont(it[4]) for it in items]))
    cb = None
    if rng is not None:
        def fill(_ctx, out, n):
            ctypes.memmove(out, bytes(rng(n)), n)
        cb = _lib.RNG_FILL(fill)
    ok = (ctypes.c_int * N)()
    all_ok = ctypes.c_int(0)
    checks = ctypes.c_size_t(0)
    st = params._L.h2_ipa_verify_proofs(params.curve, params.bases.handle, params.k, N, states, ptrs, lens, commitments.ctypes.data,
                                        x3.ctypes.data, v.ctypes.data, cb, None, ok, ctypes.byref(all_ok), ctypes.byref(checks))
    _lib.check(st, "h2_ipa_verify_proofs")
    if stats is not None:
        stats.update({"checks": int(checks.value), "all_ok": bool(all_ok.value)})
    return [bool(x) for x in ok]
