"""The lookup argument's permute and product steps over device-resident columns (include/h2hip.h:
h2_lookup_permute_device, h2_lookup_product_device).

Upstream (halo2_proofs @6b43b6b, src/plonk/lookup/prover.rs): `permute_expression_pair` sorts the compressed input
expression and arranges the compressed table expression beside it; `commit_product` builds the grand product z over the
usable rows.  Both work on m lookups per call: columns are (m, stride, 4) int64 CUDA tensors of Montgomery limbs, rows
[usable_rows, stride) are the caller's blinding rows and are never written.  Nothing leaves HBM and nothing waits: the
status words of the permute step come back as a tensor the caller reads when it wants them.
"""
import ctypes

from . import lib as _lib


def _columns(domain, t, rows):
    """(m, stride) of an (m, stride, 4) column tensor"""
    domain._shape(t, t.shape[-2])
    if t.dim() != 3:
        raise ValueError("expected shape (m, stride, 4), got %r" % (tuple(t.shape),))
    if t.shape[1] < rows:
        raise ValueError("columns of %d rows cannot hold %d" % (t.shape[1], rows))
    return int(t.shape[0]), int(t.shape[1])


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def permute_expression_pair(domain, inputs, tables, usable_rows):
    """-> (permuted_inputs, permuted_tables, status): new tensors of the shape of `inputs` whose rows [0, usable_rows) hold
    A' and S' of every pair (the other rows are zero), and an (m,) int32 tensor: 0 = done, 1 = some input value is not in
    its table (halo2's Error::ConstraintSystemFailure for that pair)."""
    import torch
    m, stride = _columns(domain, inputs, usable_rows)
    if tuple(tables.shape) != tuple(inputs.shape):
        raise ValueError("inputs and tables differ in shape")
    _columns(domain, tables, usable_rows)
    pin, ptab = torch.zeros_like(inputs), torch.zeros_like(inputs)
    status = torch.zeros((m,), dtype=torch.int32, device=inputs.device)
    st = domain._L.h2_lookup_permute_device(domain.curve, _ptr(inputs), _ptr(tables), usable_rows, stride, m, _ptr(pin),
                                            _ptr(ptab), _ptr(status), domain._stream())
    _lib.check(st, "h2_lookup_permute_device")
    return pin, ptab, status


def lookup_product(domain, inputs, tables, permuted_inputs, permuted_tables, usable_rows, beta, gamma):
    """-> z: a new tensor of the shape of `inputs` (stride >= usable_rows + 1) whose rows [0, usable_rows] hold the grand
    product of every lookup (z[0] = 1; z[usable_rows] = 1 when the lookup is satisfied), the other rows zero.  beta, gamma:
    canonical ints."""
    import torch
    m, stride = _columns(domain, inputs, usable_rows + 1)
    for t in (tables, permuted_inputs, permuted_tables):
        if tuple(t.shape) != tuple(inputs.shape):
            raise ValueError("the four column tensors differ in shape")
        _columns(domain, t, usable_rows + 1)
    z = torch.zeros_like(inputs)
    b, g = domain.mont(beta), domain.mont(gamma)
    st = domain._L.h2_lookup_product_device(domain.curve, _ptr(inputs), _ptr(tables), _ptr(permuted_inputs),
                                            _ptr(permuted_tables), usable_rows, stride, m, b.ctypes.data, g.ctypes.data,
                                            _ptr(z), domain._stream())
    _lib.check(st, "h2_lookup_product_device")
    return z
