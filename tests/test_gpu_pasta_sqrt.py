"""h2_base_sqrt_device and h2_pasta_points_decompress_device on the GPU, through ctypes as a Rust or JS host would call them:
the kernels on the inputs of tests/test_pasta_sqrt_abi.py against the same big-integer references, and the argument checks."""
import pytest

import pasta_sqrt_cases as C

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 1000]        # a partial wave, a wave boundary, several workgroups


@pytest.fixture(scope="module")
def lib(h2):
    return h2.load()


def to_mont(cid, xs):
    q = C.base_field(cid)
    R = (1 << 256) % q
    return b"".join((x * R % q if x < q else x).to_bytes(32, "little") for x in xs)


def device_sqrt(L, cid, xs, stream=None, in_place=False):
    import torch
    q, n = C.base_field(cid), len(xs)
    r_inv = pow(1 << 256, -1, q)
    d_in = torch.frombuffer(bytearray(to_mont(cid, xs)), dtype=torch.uint8).cuda()
    d_out = d_in if in_place else torch.full((32 * n,), 0xAB, dtype=torch.uint8, device="cuda")
    d_st = torch.full((n,), 0xCD, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc = L.h2_base_sqrt_device(cid, d_in.data_ptr(), n, d_out.data_ptr(), d_st.data_ptr(),
                               stream.cuda_stream if stream is not None else None)
    assert rc == 0
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    raw, st = bytes(d_out.cpu().numpy()), bytes(d_st.cpu().numpy())
    out = []
    for i in range(n):
        m = int.from_bytes(raw[32 * i:32 * i + 32], "little")
        assert m < q                                            # canonical Montgomery form, not merely congruent
        out.append((m * r_inv % q, st[i]))
    return out


@pytest.mark.parametrize("cid", [0, 1, 2])
@pytest.mark.parametrize("n", SIZES)
def test_square_root_kernel_matches_big_integers(lib, cid, n):
    import torch
    xs = C.sqrt_inputs(cid)[:n]
    got = device_sqrt(lib, cid, xs)
    for a, (root, status) in zip(xs, got):
        C.check_sqrt(cid, a, root, status)
    assert device_sqrt(lib, cid, xs, stream=torch.cuda.Stream()) == got
    assert device_sqrt(lib, cid, xs, in_place=True) == got


@pytest.mark.parametrize("cid", [1, 2])
def test_square_root_kernel_on_every_order_and_window(lib, cid):
    xs = C.sqrt_inputs(cid)                                     # all of them: every 2-power order, every window value
    for a, (root, status) in zip(xs, device_sqrt(lib, cid, xs)):
        C.check_sqrt(cid, a, root, status)


def device_decompress(L, cid, words, stream=None):
    import torch
    q, n = C.base_field(cid), len(words)
    r_inv = pow(1 << 256, -1, q)
    d_in = torch.frombuffer(bytearray(b"".join(words)), dtype=torch.uint8).cuda()
    d_out = torch.full((64 * n,), 0xAB, dtype=torch.uint8, device="cuda")
    d_st = torch.full((n,), 0xCD, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc = L.h2_pasta_points_decompress_device(cid, d_in.data_ptr(), n, d_out.data_ptr(), d_st.data_ptr(),
                                             stream.cuda_stream if stream is not None else None)
    if rc != 0:
        return rc, None
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    raw, st = bytes(d_out.cpu().numpy()), bytes(d_st.cpu().numpy())
    pts = []
    for i in range(n):
        x, y = int.from_bytes(raw[64 * i:64 * i + 32], "little"), int.from_bytes(raw[64 * i + 32:64 * i + 64], "little")
        assert x < q and y < q
        pts.append((x * r_inv % q, y * r_inv % q, st[i]))
    return 0, pts


@pytest.mark.parametrize("cid", [1, 2])
@pytest.mark.parametrize("n", SIZES)
def test_decompression_kernel_matches_transcript(lib, cid, n):
    import torch
    mix = C.decompress_mix(cid)
    words = [mix[i % len(mix)] for i in range(n)]
    rc, got = device_decompress(lib, cid, words)
    assert rc == 0
    for w, g in zip(words, got):
        assert g == C.expected_point(cid, w), (w.hex(), g)
    assert device_decompress(lib, cid, words, stream=torch.cuda.Stream()) == (0, got)
    if n >= len(mix):
        assert {g[2] for g in got} == {0, 1, 2, 3}


def test_argument_checks(lib):
    import torch
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    p = buf.data_ptr()
    sq, de = lib.h2_base_sqrt_device, lib.h2_pasta_points_decompress_device
    assert device_decompress(lib, 0, C.decompress_mix(1)[:4]) == (-1, None)          # BN254 has its own wire form
    assert sq(3, p, 1, p + 64, p + 128, None) == -1 and de(3, p, 1, p + 64, p + 128, None) == -1       # unknown curve
    for fn in (sq, de):
        assert fn(1, None, 1, p + 64, p + 128, None) == -1                           # null pointers with n > 0
        assert fn(1, p, 1, None, p + 128, None) == -1
        assert fn(1, p, 1, p + 64, None, None) == -1
        assert fn(1, p + 4, 1, p + 64, p + 128, None) == -1                          # not 16-byte aligned
        assert fn(1, p, 1, p + 64 + 8, p + 128, None) == -1
        assert fn(1, p, (1 << 30) + 1, p + 64, p + 128, None) == -1                  # n > 2^30
        assert fn(1, None, 0, None, None, None) == 0                                 # n = 0 enqueues nothing
        assert fn(1, p, 4, p + 16, p + 1024, None) == -1                             # an output partly over the input
        assert fn(1, p, 4, p + 1024, p + 8, None) == -1                              # the status bytes over the input
    assert sq(1, p, 4, p, p + 1024, None) == 0                                       # exactly in place: allowed
    assert de(1, p, 4, p, p + 1024, None) == -1                                      # 64 bytes out per 32 in: never in place
    torch.cuda.synchronize()
