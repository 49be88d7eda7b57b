"""Poseidon over device-resident columns (include/h2hip.h: h2_poseidon_*).

The primitive of the reference's circuits/src/poseidon/primitives*: width 3, rate 2, S-box x^5, r_f full and r_p partial
rounds over the scalar field of a curve, constants from the Grain / Cauchy-MDS generation.  The defaults are the two
instances the reference uses: (8, 56) on Pallas and Vesta (P128Pow5T3, the zcash vectors) and (8, 60) on BN254
(poseidon_circuit.rs's spec: the hash the Poseidon circuit proves).

`width=5` and `width=9` (rate 4 and 8; h2_poseidon_wide_*) are the same primitive for 4-ary and 8-ary hashes and trees.
They have no default rounds: r_f and r_p must be given.  Every width goes through the width-taking entry points
(h2_poseidon_wide_*); the h2_poseidon_* names are those calls at width 3.

Elements are 4 x u64 Montgomery limbs, canonical.  The device functions take int64 CUDA tensors viewing those limbs, or
numpy uint64 arrays, which are uploaded, and return the same kind: the work is enqueued on the caller's current stream
and the columns stay in HBM.  There is no CPU fallback: `merkle_path` and `verify_path` are host helpers on Python
integers for a membership proof's few hashes, everything else runs the kernels.  `merkle_paths`, `verify_paths` and
`merkle_update` are their device counterparts on a resident tree: many paths per call, indices as uint32 (numpy) or int32
CUDA tensors, one status word per item.
"""
import ctypes

import numpy as np

from . import lib as _lib
from .api import _curve_id, _ensure_init
from .domain import _FIELDS, _limbs

DEFAULT_ROUNDS = {0: (8, 60), 1: (8, 56), 2: (8, 56)}


def _rounds(curve, r_f, r_p, width=3):
    if width != 3:
        if width not in (5, 9):
            raise ValueError("poseidon: width must be 3, 5 or 9")
        if r_f is None or r_p is None:
            raise ValueError("poseidon: width %d has no default rounds, give r_f and r_p" % width)
        return int(r_f), int(r_p)
    d = DEFAULT_ROUNDS[curve]
    return (d[0] if r_f is None else int(r_f), d[1] if r_p is None else int(r_p))


def _arity_depth(n, width):
    """depth with (width - 1)^depth == n, or None"""
    a, depth, m = width - 1, 0, 1
    while m < n:
        m *= a
        depth += 1
    return depth if m == n and depth >= 1 else None


def modulus(curve):
    return _FIELDS[_curve_id(curve)][0]


def to_mont(curve, values):
    """canonical ints -> (n, 4) uint64 Montgomery limbs"""
    p = modulus(curve)
    R = (1 << 256) % p
    return np.stack([_limbs(int(v) % p * R % p) for v in values]) if len(values) else np.zeros((0, 4), dtype=np.uint64)


def from_mont(curve, limbs):
    """Montgomery limbs (any shape ending in 4) -> a flat list of canonical ints"""
    p = modulus(curve)
    r_inv = pow((1 << 256) % p, -1, p)
    raw = np.ascontiguousarray(limbs, dtype=np.uint64).tobytes()
    return [int.from_bytes(raw[i:i + 32], "little") * r_inv % p for i in range(0, len(raw), 32)]


def constants(curve, r_f=None, r_p=None, as_int=False, width=3):
    """The instance's constants, host only (no GPU): (round constants (r_f + r_p, width, 4), mds (width, width, 4)) as
    Montgomery limbs, or as nested lists of canonical ints with as_int."""
    cid = _curve_id(curve)
    r_f, r_p = _rounds(cid, r_f, r_p, width)
    L = _lib.load()
    need = ctypes.c_size_t(0)

    def call(out, cap):
        return L.h2_poseidon_wide_constants(cid, width, r_f, r_p, out, cap, ctypes.byref(need))
    call(None, 0)
    if need.value == 0:
        raise ValueError("poseidon: r_f must be even and at least 2, r_f + r_p at most 128")
    out = np.zeros((need.value, 4), dtype=np.uint64)
    _lib.check(call(out.ctypes.data, need.value), "h2_poseidon_wide_constants")
    rounds, t = r_f + r_p, width
    rcs, mds = out[:t * rounds].reshape(rounds, t, 4), out[t * rounds:].reshape(t, t, 4)
    if not as_int:
        return rcs, mds
    ri, mi = from_mont(cid, rcs), from_mont(cid, mds)
    return [ri[t * r:t * r + t] for r in range(rounds)], [mi[t * i:t * i + t] for i in range(t)]


def _stream():
    import torch
    raw = getattr(torch._C, "_cuda_getCurrentRawStream", None)
    if raw is not None:
        return ctypes.c_void_p(raw(torch.cuda.current_device()))
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _device(a, name):
    """(tensor, was_numpy): an int64 CUDA tensor viewing the limbs"""
    import torch
    if isinstance(a, torch.Tensor):
        if a.dtype != torch.int64 or not a.is_cuda or not a.is_contiguous():
            raise ValueError("%s: expected a contiguous int64 CUDA tensor" % name)
        return a, False
    a = np.ascontiguousarray(a, dtype=np.uint64)
    return torch.from_numpy(a.view(np.int64).copy()).cuda(), True


def _result(t, was_numpy):
    return t.cpu().numpy().view(np.uint64) if was_numpy else t


def permute(curve, states, r_f=None, r_p=None, out=None, width=3):
    """n states (n, width, 4) -> the permuted states.  `out` (a tensor of the same shape) may be `states` itself."""
    import torch
    _ensure_init()
    cid = _curve_id(curve)
    r_f, r_p = _rounds(cid, r_f, r_p, width)
    d_in, was_numpy = _device(states, "states")
    if d_in.dim() != 3 or tuple(d_in.shape[1:]) != (width, 4):
        raise ValueError("states: expected shape (n, %d, 4), got %r" % (width, tuple(d_in.shape)))
    d_out = torch.empty_like(d_in) if out is None else out
    if tuple(d_out.shape) != tuple(d_in.shape) or d_out.dtype != torch.int64 or not d_out.is_cuda or not d_out.is_contiguous():
        raise ValueError("out: expected a contiguous int64 CUDA tensor of the states' shape")
    st = _lib.load().h2_poseidon_wide_permute_device(cid, width, r_f, r_p, ctypes.c_void_p(d_in.data_ptr()),
                                                     ctypes.c_void_p(d_out.data_ptr()), d_in.shape[0], _stream())
    _lib.check(st, "h2_poseidon_wide_permute_device")
    return _result(d_out, was_numpy)


def hash(curve, msgs, r_f=None, r_p=None, length=None, width=3):  # noqa: A001 -- the primitive's name
    """ConstantLength hash of n messages at rate width - 1: msgs (n, stride, 4), the first `length` elements of each row
    are the message (default: the whole row) -> (n, 4)."""
    import torch
    _ensure_init()
    cid = _curve_id(curve)
    r_f, r_p = _rounds(cid, r_f, r_p, width)
    d_in, was_numpy = _device(msgs, "msgs")
    if d_in.dim() != 3 or d_in.shape[2] != 4 or d_in.shape[1] == 0:
        raise ValueError("msgs: expected shape (n, stride, 4), got %r" % (tuple(d_in.shape),))
    n, stride = d_in.shape[0], d_in.shape[1]
    length = stride if length is None else int(length)
    d_out = torch.empty((n, 4), dtype=torch.int64, device=d_in.device)
    st = _lib.load().h2_poseidon_wide_hash_device(cid, width, r_f, r_p, ctypes.c_void_p(d_in.data_ptr()), length, stride, n,
                                                  ctypes.c_void_p(d_out.data_ptr()), _stream())
    _lib.check(st, "h2_poseidon_wide_hash_device")
    return _result(d_out, was_numpy)


def merkle_nodes(curve, leaves, r_f=None, r_p=None, width=3):
    """a^depth leaves (a^depth, 4), a = width - 1, depth >= 1 -> the (a^depth - 1) / (a - 1) inner nodes, level by level
    from the leaves' parents up; the root is last.  A node is the ConstantLength<a> hash of its a children."""
    import torch
    _ensure_init()
    cid = _curve_id(curve)
    r_f, r_p = _rounds(cid, r_f, r_p, width)
    d_in, was_numpy = _device(leaves, "leaves")
    n = d_in.shape[0] if d_in.dim() == 2 else 0
    depth = _arity_depth(n, width)
    if d_in.dim() != 2 or d_in.shape[1] != 4 or depth is None:
        raise ValueError("leaves: expected shape (%d^depth, 4) with depth >= 1, got %r" % (width - 1, tuple(d_in.shape)))
    d_out = torch.empty(((n - 1) // (width - 2), 4), dtype=torch.int64, device=d_in.device)
    st = _lib.load().h2_poseidon_wide_merkle_device(cid, width, r_f, r_p, ctypes.c_void_p(d_in.data_ptr()), depth,
                                                    ctypes.c_void_p(d_out.data_ptr()), _stream())
    _lib.check(st, "h2_poseidon_wide_merkle_device")
    return _result(d_out, was_numpy)


def merkle_root(curve, leaves, r_f=None, r_p=None, width=3):
    """the root alone: (4,) limbs"""
    return merkle_nodes(curve, leaves, r_f, r_p, width)[-1]


def merkle_tail():
    """the widest level merkle_nodes leaves to its single-workgroup launch"""
    return _lib.load().h2_poseidon_merkle_tail()


# ---- a resident tree: paths, verification, update -------------------------------------------------------------------------
STATUS_OK, STATUS_RANGE, STATUS_NONCANONICAL, STATUS_SUPERSEDED, STATUS_MISMATCH = 0, 1, 2, 3, 4


def _device_u32(a, name):
    """(tensor, was_numpy): an int32 CUDA tensor viewing uint32 words"""
    import torch
    if isinstance(a, torch.Tensor):
        if a.dtype != torch.int32 or not a.is_cuda or not a.is_contiguous() or a.dim() != 1:
            raise ValueError("%s: expected a contiguous one-dimensional int32 CUDA tensor" % name)
        return a, False
    a = np.ascontiguousarray(a, dtype=np.uint32).reshape(-1)
    return torch.from_numpy(a.view(np.int32).copy()).cuda(), True


def _status(t, as_numpy):
    return t.cpu().numpy().view(np.uint32) if as_numpy else t


def _tree(leaves, nodes, width=3):
    """(d_leaves, d_nodes, depth, were_numpy) of a tree as merkle_nodes lays it out"""
    d_leaves, np_l = _device(leaves, "leaves")
    d_nodes, np_n = _device(nodes, "nodes")
    n = d_leaves.shape[0] if d_leaves.dim() == 2 else 0
    depth = _arity_depth(n, width)
    if d_leaves.dim() != 2 or d_leaves.shape[1] != 4 or depth is None:
        raise ValueError("leaves: expected shape (%d^depth, 4) with depth >= 1, got %r" % (width - 1, tuple(d_leaves.shape)))
    if tuple(d_nodes.shape) != ((n - 1) // (width - 2), 4):
        raise ValueError("nodes: expected shape (%d, 4), got %r" % ((n - 1) // (width - 2), tuple(d_nodes.shape)))
    return d_leaves, d_nodes, depth, np_l or np_n


def merkle_paths(curve, leaves, nodes, indices, width=3):
    """The membership paths of n leaves of a resident tree, cut on the device: (paths (n, depth, 4), status (n,)); at
    widths 5 and 9 paths (n, depth * (width - 2), 4).  paths[i] is merkle_path_wide's list for indices[i] (width 3: merkle_path's);
    an index >= a^depth gives status 1 and a zero path."""
    import torch
    _ensure_init()
    cid = _curve_id(curve)
    if width not in (3, 5, 9):
        raise ValueError("poseidon: width must be 3, 5 or 9")
    d_leaves, d_nodes, depth, np_tree = _tree(leaves, nodes, width)
    d_idx, np_idx = _device_u32(indices, "indices")
    n = d_idx.shape[0]
    d_paths = torch.empty((n, depth * (width - 2), 4), dtype=torch.int64, device=d_leaves.device)
    d_status = torch.empty((n,), dtype=torch.int32, device=d_leaves.device)
    if n:   # an empty tensor has no address to pass: n = 0 is the C call's H2_OK, nothing enqueued
        st = _lib.load().h2_poseidon_wide_merkle_paths_device(cid, width, ctypes.c_void_p(d_leaves.data_ptr()),
                                                              ctypes.c_void_p(d_nodes.data_ptr()), depth, ctypes.c_void_p(d_idx.data_ptr()),
                                                              n, ctypes.c_void_p(d_paths.data_ptr()), ctypes.c_void_p(d_status.data_ptr()),
                                                              _stream())
        _lib.check(st, "h2_poseidon_wide_merkle_paths_device")
    as_numpy = np_tree and np_idx
    return _result(d_paths, as_numpy), _status(d_status, as_numpy)


def verify_paths(curve, leaf_values, indices, paths, root=None, r_f=None, r_p=None, width=3):
    """n membership paths (n, depth * (width - 2), 4) walked on the device: (roots (n, 4), status (n,)).  Status 0: index in range, every element
    canonical and -- when `root` (4 limbs) is given -- the computed root equals it; 1: index out of range; 2: an element not
    canonical (never reduced silently); 4: another root.  Items with status 1 or 2 get a zero root."""
    import torch
    _ensure_init()
    cid = _curve_id(curve)
    r_f, r_p = _rounds(cid, r_f, r_p, width)
    d_leafs, np_v = _device(leaf_values, "leaf_values")
    d_paths, np_p = _device(paths, "paths")
    d_idx, np_i = _device_u32(indices, "indices")
    n = d_idx.shape[0]
    if (d_paths.dim() != 3 or d_paths.shape[0] != n or (n and d_paths.shape[1] == 0) or d_paths.shape[1] % (width - 2)
            or d_paths.shape[2] != 4):
        raise ValueError("paths: expected shape (%d, depth * %d, 4) with depth >= 1, got %r" % (n, width - 2, tuple(d_paths.shape)))
    if tuple(d_leafs.shape) != (n, 4):
        raise ValueError("leaf_values: expected shape (%d, 4), got %r" % (n, tuple(d_leafs.shape)))
    depth = d_paths.shape[1] // (width - 2)
    d_root = None
    if root is not None:
        d_root = _device(root, "root")[0]
        if d_root.numel() != 4:
            raise ValueError("root: expected one element of 4 limbs")
    d_roots = torch.empty((n, 4), dtype=torch.int64, device=d_paths.device)
    d_status = torch.empty((n,), dtype=torch.int32, device=d_paths.device)
    if n:
        st = _lib.load().h2_poseidon_wide_merkle_verify_device(cid, width, r_f, r_p, ctypes.c_void_p(d_leafs.data_ptr()),
                                                               ctypes.c_void_p(d_idx.data_ptr()), ctypes.c_void_p(d_paths.data_ptr()),
                                                               depth, n, None if d_root is None else ctypes.c_void_p(d_root.data_ptr()),
                                                               ctypes.c_void_p(d_roots.data_ptr()), ctypes.c_void_p(d_status.data_ptr()),
                                                               _stream())
        _lib.check(st, "h2_poseidon_wide_merkle_verify_device")
    as_numpy = np_v and np_p and np_i
    return _result(d_roots, as_numpy), _status(d_status, as_numpy)


def merkle_update(curve, leaves, nodes, indices, values, r_f=None, r_p=None):
    """leaves[indices[i]] = values[i] IN PLACE on the device tensors `leaves` (2^depth, 4) and `nodes` (2^depth - 1, 4), the
    nodes above the written leaves hashed again -> status (n,).  1: index out of range, 2: value not canonical (both
    dropped), 3: a later item writes the same leaf (the last one is stored), 0: stored."""
    import torch
    _ensure_init()
    cid = _curve_id(curve)
    r_f, r_p = _rounds(cid, r_f, r_p)
    if not isinstance(leaves, torch.Tensor) or not isinstance(nodes, torch.Tensor):
        raise ValueError("merkle_update: leaves and nodes are updated in place and must be CUDA tensors")
    d_leaves, d_nodes, depth, _ = _tree(leaves, nodes)
    d_idx, np_i = _device_u32(indices, "indices")
    d_val, np_v = _device(values, "values")
    n = d_idx.shape[0]
    if tuple(d_val.shape) != (n, 4):
        raise ValueError("values: expected shape (%d, 4), got %r" % (n, tuple(d_val.shape)))
    d_status = torch.empty((n,), dtype=torch.int32, device=d_leaves.device)
    if n:
        st = _lib.load().h2_poseidon_merkle_update_device(cid, r_f, r_p, ctypes.c_void_p(d_leaves.data_ptr()),
                                                          ctypes.c_void_p(d_nodes.data_ptr()), depth, ctypes.c_void_p(d_idx.data_ptr()),
                                                          ctypes.c_void_p(d_val.data_ptr()), n, ctypes.c_void_p(d_status.data_ptr()),
                                                          _stream())
        _lib.check(st, "h2_poseidon_merkle_update_device")
    return _status(d_status, np_i and np_v)


# ---- host helpers on Python integers, for a membership proof's few hashes ------------------------------------------------
def merkle_path_wide(nodes, arity, depth, index):
    """The siblings of leaf `index` from the bottom up, arity - 1 per level in child order with the ancestor's own position
    left out.  nodes: the whole tree as canonical ints, the arity^depth leaves followed by merkle_nodes' inner nodes."""
    total = (arity ** (depth + 1) - 1) // (arity - 1)
    if len(nodes) != total or not 0 <= index < arity ** depth:
        raise ValueError("merkle_path_wide: expected (arity^(depth + 1) - 1) / (arity - 1) nodes and an index below arity^depth")
    path, base, width = [], 0, arity ** depth
    for _ in range(depth):
        first = index - index % arity
        path.extend(nodes[base + first + c] for c in range(arity) if first + c != index)
        base += width
        width //= arity
        index //= arity
    return path


def hashn_int(curve, words, r_f, r_p):
    """ConstantLength<len(words)> of canonical ints at width len(words) + 1 on the host (big integers, one permutation)"""
    cid = _curve_id(curve)
    t = len(words) + 1
    r_f, r_p = _rounds(cid, r_f, r_p, t)
    p = modulus(cid)
    rcs, mds = constants(cid, r_f, r_p, as_int=True, width=t)
    st = [w % p for w in words] + [(len(words) << 64) % p]
    half = r_f // 2
    for r in range(r_f + r_p):
        st = [(st[i] + rcs[r][i]) % p for i in range(t)]
        if r < half or r >= half + r_p:
            st = [pow(x, 5, p) for x in st]
        else:
            st[0] = pow(st[0], 5, p)
        st = [sum(mds[i][j] * st[j] for j in range(t)) % p for i in range(t)]
    return st[0]


def verify_path_wide(curve, arity, leaf, index, path, root, r_f, r_p):
    """True when `path` (merkle_path_wide's siblings) takes `leaf` at position `index` to `root`"""
    if len(path) % (arity - 1):
        return False
    cur = leaf
    for l in range(len(path) // (arity - 1)):
        sibs = list(path[l * (arity - 1):(l + 1) * (arity - 1)])
        sibs.insert(index % arity, cur)
        cur = hashn_int(curve, sibs, r_f, r_p)
        index //= arity
    return index == 0 and cur == root


# ---- the same at arity 2 (width 3, which has default rounds) ------------------------------------------------------------
def merkle_path(nodes, depth, index):
    """The siblings of leaf `index` from the bottom up.  nodes: the whole tree as canonical ints, the 2^depth leaves
    followed by merkle_nodes' 2^depth - 1 inner nodes (2^(depth + 1) - 1 values)."""
    return merkle_path_wide(nodes, 2, depth, index)


def hash2_int(curve, a, b, r_f=None, r_p=None):
    """ConstantLength<2> of two canonical ints on the host"""
    return hashn_int(curve, [a, b], r_f, r_p)


def verify_path(curve, leaf, index, path, root, r_f=None, r_p=None):
    """True when `path` (merkle_path's siblings) takes `leaf` at position `index` to `root`"""
    return verify_path_wide(curve, 2, leaf, index, path, root, r_f, r_p)
