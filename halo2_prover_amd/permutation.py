"""The permutation argument's grand products over device-resident columns (include/h2hip.h:
h2_permutation_product_device).

Upstream (halo2_proofs @6b43b6b, src/plonk/permutation/prover.rs `Argument::commit`): the permutation columns are cut into
sets of chunk_len = cs.degree() - 2; every set's z starts at the last usable value of the set before it.  One call builds
all sets of all instances: the sets of an instance are one running product on the device, so no tail is read back.  Rows
(usable_rows, n) of every z column -- the blinding rows -- and the RNG draws that fill them stay the caller's.
"""
import ctypes

import numpy as np

from . import lib as _lib


def _column(t, rows):
    if t.dtype.__str__() != "torch.int64" or not t.is_cuda or not t.is_contiguous() or t.dim() != 2 or t.shape[1] != 4:
        raise ValueError("columns must be contiguous (rows, 4) int64 CUDA tensors")
    if t.shape[0] < rows:
        raise ValueError("a column of %d rows cannot hold %d" % (t.shape[0], rows))
    return t.data_ptr()


def permutation_product(domain, values, sigma, chunk_len, usable_rows, betas, gammas, omega, delta):
    """-> z: a new (m, S, domain.n, 4) tensor, S = ceil(n_cols / chunk_len); rows [0, usable_rows] of z[p][s] hold the
    grand product of set s of instance p (z[p][0][0] = 1, z[p][s + 1][0] = z[p][s][usable_rows]; z[p][S - 1][usable_rows]
    = 1 when the copy constraints hold), the other rows are zero.
    values: m lists of n_cols column tensors ((rows, 4) int64 CUDA, rows >= usable_rows), one list per instance;
    sigma: the n_cols permutation columns of the key, Lagrange form, shared; betas, gammas: m canonical ints each;
    omega, delta: canonical ints (the domain's generator and halo2's DELTA)."""
    import torch
    m, n_cols = len(values), len(sigma)
    if len(betas) != m or len(gammas) != m:
        raise ValueError("expected one beta and one gamma per instance")
    if any(len(v) != n_cols for v in values):
        raise ValueError("every instance needs %d columns" % n_cols)
    if chunk_len < 1 or not 0 <= usable_rows < domain.n:
        raise ValueError("chunk_len >= 1 and usable_rows < n are required")
    S = (n_cols + chunk_len - 1) // chunk_len
    device = sigma[0].device if n_cols else "cuda"
    z = torch.zeros((m, S, domain.n, 4), dtype=torch.int64, device=device)
    if m == 0 or n_cols == 0:
        return z
    vp = (ctypes.c_void_p * (m * n_cols))(*[_column(c, usable_rows) for v in values for c in v])
    sp = (ctypes.c_void_p * n_cols)(*[_column(c, usable_rows) for c in sigma])
    b = np.concatenate([domain.mont(x) for x in betas])
    g = np.concatenate([domain.mont(x) for x in gammas])
    w, d = domain.mont(omega), domain.mont(delta)
    st = domain._L.h2_permutation_product_device(domain.curve, vp, sp, n_cols, chunk_len, usable_rows, m, b.ctypes.data,
                                                 g.ctypes.data, w.ctypes.data, d.ctypes.data,
                                                 ctypes.c_void_p(z.data_ptr()), domain.n, domain._stream())
    _lib.check(st, "h2_permutation_product_device")
    return z
