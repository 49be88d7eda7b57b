"""CPU (no GPU): the ABI of h2_ipa_* -- exported by the built library, listed by the Python loader with their argument
lists, declared in include/h2hip.h; h2_version() did not move (a host detects the entry points by their symbols); the
state's size is known without a device; the host helpers compute_s / compute_b match their definitions."""
import ctypes
import os
import random
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_P, _Z, _I, _U32, _U64 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint64
ARGS = {
    # k, out
    "h2_ipa_state_bytes": [_U32, ctypes.POINTER(_Z)],
    # curve, k, d_p, x3, d_state, stream
    "h2_ipa_begin_device": [_I, _U32, _P, _P, _P, _P],
    # curve, bases, k, j, d_state, u_prev, u_prev_inv, z, l_blind, r_blind, d_out_affine, stream
    "h2_ipa_round_device": [_I, _U64, _U32, _U32, _P, _P, _P, _P, _P, _P, _P, _P],
    # curve, k, d_state, u_last, u_last_inv, d_out, d_s_out, stream
    "h2_ipa_final_device": [_I, _U32, _P, _P, _P, _P, _P, _P],
    # curve, u, k, init, d_out, stream
    "h2_ipa_challenge_products_device": [_I, _P, _U32, _P, _P, _P],
}
PRIMES = [0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001,
          0x40000000000000000000000000000000224698FC0994A8DD8C46EB2100000001,
          0x40000000000000000000000000000000224698FC094CF91B992D30ED00000001]


@pytest.mark.parametrize("name", sorted(ARGS))
def test_library_exports_the_entry_point(name):
    import halo2_prover_amd
    lib = halo2_prover_amd.load()
    assert hasattr(lib, name)
    assert lib.h2_version() == 1002


@pytest.mark.parametrize("name", sorted(ARGS))
def test_loader_lists_it_with_its_arguments(name):
    import halo2_prover_amd
    res, args = halo2_prover_amd.SYMBOLS[name]
    assert res is ctypes.c_int and args == ARGS[name]


@pytest.mark.parametrize("name", sorted(ARGS))
def test_header_declares_it(name):
    text = open(os.path.join(ROOT, "include", "h2hip.h")).read()
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, "include/h2hip.h does not declare " + name
    assert len(m.group(1).split(",")) == len(ARGS[name])


def max_k():
    text = open(os.path.join(ROOT, "include", "h2hip.h")).read()
    return int(re.search(r"#define\s+H2_IPA_MAX_K\s+(\d+)", text).group(1))


def test_the_header_states_a_maximum_of_at_least_16():
    assert max_k() >= 16


def test_state_bytes_grows_with_k_and_refuses_the_ends():
    import halo2_prover_amd
    lib = halo2_prover_amd.load()
    out = ctypes.c_size_t(0)
    sizes = []
    for k in range(1, max_k() + 1):
        assert lib.h2_ipa_state_bytes(k, ctypes.byref(out)) == 0
        n = 1 << k
        # a, b and s of n elements each and two columns of n + 2, 32 bytes an element, at the least
        assert out.value >= 32 * (3 * n + 2 * (n + 2)) and out.value % 32 == 0
        sizes.append(out.value)
    assert all(a < b for a, b in zip(sizes, sizes[1:]))
    assert lib.h2_ipa_state_bytes(0, ctypes.byref(out)) == -1
    assert lib.h2_ipa_state_bytes(max_k() + 1, ctypes.byref(out)) == -1
    assert lib.h2_ipa_state_bytes(4, None) == -1


@pytest.mark.parametrize("k", [1, 2, 7, "max"])
def test_the_single_state_is_the_batch_state_of_one(k):
    import halo2_prover_amd
    lib = halo2_prover_amd.load()
    k = max_k() if k == "max" else k
    one, batch = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert lib.h2_ipa_state_bytes(k, ctypes.byref(one)) == 0
    assert lib.h2_ipa_batch_state_bytes(k, 1, ctypes.byref(batch)) == 0
    assert one.value == batch.value > 0


def test_they_fail_loudly_without_init():
    """no CPU fallback: before h2_init the calls are H2_ENOTINIT (H2_EINVAL's null pointers if another test of this
    process has initialised a device)"""
    import halo2_prover_amd
    lib = halo2_prover_amd.load()
    c = (ctypes.c_uint64 * 4)(1, 0, 0, 0)
    assert lib.h2_ipa_begin_device(1, 4, None, c, None, None) in (-5, -1)
    assert lib.h2_ipa_round_device(1, 1, 4, 0, None, None, None, c, c, c, None, None) in (-5, -1)
    assert lib.h2_ipa_final_device(1, 4, None, c, c, None, None, None) in (-5, -1)
    assert lib.h2_ipa_challenge_products_device(1, c, 1, c, None, None) in (-5, -1)


def test_the_python_layer_exports_the_argument():
    import halo2_prover_amd
    assert callable(halo2_prover_amd.ParamsIPA) and callable(halo2_prover_amd.ipa.create_proof)
    assert callable(halo2_prover_amd.ipa.verify_proof) and callable(halo2_prover_amd.Blake2bTranscript)


@pytest.mark.parametrize("k", [1, 2, 5])
@pytest.mark.parametrize("p", PRIMES)
def test_compute_s_and_compute_b_match_their_definitions(k, p):
    from halo2_prover_amd.ipa import compute_b, compute_s
    rnd = random.Random(0x1BA0 + k)
    u = [rnd.randrange(1, p) for _ in range(k)]
    init = rnd.randrange(1, p)
    x = rnd.randrange(p)
    s = compute_s(u, init, p)
    assert len(s) == 1 << k
    for i in range(1 << k):
        want = init
        for t in range(k):
            if (i >> t) & 1:
                want = want * u[k - 1 - t] % p
        assert s[i] == want
    want_b = 1
    for t in range(k):
        want_b = want_b * (1 + u[k - 1 - t] * pow(x, 1 << t, p)) % p
    assert compute_b(x, u, p) == want_b
    s1 = compute_s(u, 1, p)
    assert compute_b(x, u, p) == sum(si * pow(x, i, p) for i, si in enumerate(s1)) % p


def test_pasta_points_round_trip_through_the_wire_form():
    """x little-endian with the parity of y in bit 255; the identity is 32 zero bytes"""
    from halo2_prover_amd.transcript import FIELDS, compress, decompress, sqrt_mod
    for cid in (1, 2):
        _, q, b = FIELDS[cid]
        x = 1
        while sqrt_mod(x ** 3 + b, q) is None:
            x += 1
        y = sqrt_mod(x ** 3 + b, q)
        for pt in ((x, y), (x, q - y)):
            enc = compress(cid, pt)
            assert enc[31] >> 7 == pt[1] & 1 and decompress(cid, enc) == pt
        assert compress(cid, None) == bytes(32) and decompress(cid, bytes(32)) is None
