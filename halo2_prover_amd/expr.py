"""Expressions over device-resident columns (include/h2hip.h: h2_expr_compile, h2_expr_eval_device).

Upstream (halo2_proofs @6b43b6b, src/plonk/evaluation.rs `evaluate_h`): every gate, the permutation terms and the lookup
terms, folded by y, on every row of the extended domain.  Here the host describes that expression once as a DAG; the
library compiles it to a straight-line program and one kernel launch evaluates it for m instances (proofs), whatever
the number of nodes.  Columns are (rows, 4) int64 CUDA tensors of Montgomery limbs and stay in HBM; challenges are
variables, set per call.  Compiling needs no GPU.
"""
import ctypes
import struct

import numpy as np

from . import lib as _lib
from .api import _curve_id
from .domain import _FIELDS, _limbs

CONST, COL, ADD, SUB, MUL, VAR = 0, 1, 2, 3, 4, 5


class ExprProgram:
    """nodes: (op, a, b, x) tuples -- (CONST, 0, 0, k) constant number k | (COL, c, 0, rot) column c at a rotation in
    [-128, 127] | (ADD / SUB / MUL, a, b, 0) of the EARLIER nodes a and b | (VAR, 0, 0, v) variable number v; the last
    node is the root.  consts: canonical ints.  Negated is 0 - a, Scaled a product with a constant."""

    def __init__(self, nodes, consts, n_cols, n_vars, curve="bn254"):
        self.handle = None
        self.curve = _curve_id(curve)
        self.p = _FIELDS[self.curve][0]
        self.R = (1 << 256) % self.p
        self.n_cols, self.n_vars = n_cols, n_vars
        self._L = _lib.load()
        raw = b"".join(struct.pack("<4i", *nd) for nd in nodes)
        cm = np.concatenate([self._mont(c) for c in consts]) if len(consts) else np.zeros(0, dtype=np.uint64)
        h = ctypes.c_uint64(0)
        st = self._L.h2_expr_compile(self.curve, raw, len(nodes), cm.ctypes.data if len(consts) else None, len(consts),
                                     n_cols, n_vars, ctypes.byref(h))
        _lib.check(st, "h2_expr_compile")
        self.handle = h.value

    def _mont(self, v):
        if not 0 <= v < self.p:
            raise ValueError("not a canonical field element")
        return _limbs(v * self.R % self.p)

    def info(self):
        """the program's counters as a dict: instructions, products, column_reads, slots, constants, reductions, n_cols,
        n_vars, lds_bytes, min_rot, max_rot, curve"""
        out = _lib.ExprInfo()
        _lib.check(self._L.h2_expr_info(self.handle, ctypes.byref(out)), "h2_expr_info")
        return {name: int(getattr(out, name)) for name, _ in _lib.ExprInfo._fields_}

    def dump(self):
        """the compiled program as bytes: six u32 counters, the code (12 bytes per instruction), the constant table (32
        canonical little-endian bytes each), the table index of each variable (u32)"""
        n = ctypes.c_size_t(0)
        self._L.h2_expr_dump(self.handle, None, 0, ctypes.byref(n))
        buf = ctypes.create_string_buffer(max(1, n.value))
        _lib.check(self._L.h2_expr_dump(self.handle, buf, n.value, ctypes.byref(n)), "h2_expr_dump")
        return buf.raw[:n.value]

    def release(self):
        """give the handle and its device code back; also done when the object is collected or leaves a `with` block"""
        if self.handle is not None:
            h, self.handle = self.handle, None
            _lib.check(self._L.h2_expr_release(h), "h2_expr_release")

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.release()

    def __del__(self):
        if getattr(self, "handle", None) is not None:      # a constructor that raised has no handle
            try:
                self._L.h2_expr_release(self.handle)
            except Exception:                              # interpreter shutdown: the library may be gone
                pass
            self.handle = None

    def eval(self, domain, cols, vars, log_rows, rot_step, out=None, out_stride=None):
        """cols: m lists of n_cols column tensors ((2^log_len, 4) int64, log_len <= log_rows, the same lengths for every
        instance); vars: m lists of n_vars canonical ints.  -> a new (m, 2^log_rows, 4) tensor: on row i the root's value
        with column c at rotation r read at row (i + r * rot_step) mod its length.  One launch on the current stream.
        (out, out_stride: write into rows [0, 2^log_rows) of the columns of an existing (m, out_stride, 4) tensor.)"""
        import torch
        m, rows = len(cols), 1 << log_rows
        if domain.curve != self.curve:
            raise ValueError("the domain is over another curve")
        if len(vars) != m or any(len(v) != self.n_vars for v in vars) or any(len(c) != self.n_cols for c in cols):
            raise ValueError("expected %d lists of %d columns and of %d variables" % (m, self.n_cols, self.n_vars))
        log_len = np.zeros(max(1, self.n_cols), dtype=np.uint32)
        for p in range(m):
            for c, t in enumerate(cols[p]):
                domain._shape(t, t.shape[-2])
                n = int(t.numel() // 4)
                if n == 0 or n & (n - 1) or (p and log_len[c] != n.bit_length() - 1):
                    raise ValueError("column %d of instance %d: %d rows" % (c, p, n))
                log_len[c] = n.bit_length() - 1
        ptrs = (ctypes.c_void_p * max(1, m * self.n_cols))(*[t.data_ptr() for inst in cols for t in inst])
        vm = (np.concatenate([self._mont(x) for inst in vars for x in inst]) if m * self.n_vars
              else np.zeros(4, dtype=np.uint64))
        if out is None:
            out_stride = rows
            out = torch.empty((m, rows, 4), dtype=torch.int64, device="cuda")
        else:
            if out_stride is None or out_stride < rows or out.dim() != 3 or tuple(out.shape) != (m, out_stride, 4):
                raise ValueError("out must have shape (%d, out_stride >= %d, 4), got %r with out_stride %r"
                                 % (m, rows, tuple(out.shape), out_stride))
            domain._shape(out, out_stride)           # a contiguous int64 CUDA tensor
        st = self._L.h2_expr_eval_device(self.handle, ptrs, log_len.ctypes.data, vm.ctypes.data, m, log_rows, rot_step,
                                         ctypes.c_void_p(out.data_ptr()), out_stride, domain._stream())
        _lib.check(st, "h2_expr_eval_device")
        return out
