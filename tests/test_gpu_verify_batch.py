"""h2_verify_proofs and h2_points_decompress_device on the GPU, through ctypes as a Rust or JS host would call them.

The judge of every batch is the single verifier: ok[i] must be what h2_verify_proof says about item i alone, whatever
the neighbours are.  The decompression kernel is compared with Python big integers on the input mix of
tests/test_verify_batch.py.  Exact values throughout.
"""
import ctypes
import math
import random

import pytest

from test_capi_product import (ARITH_INPUT, COLLATZ_INPUT, POSEIDON_INPUT, Stream, c_prove, c_setup, c_verify, golden)
from test_verify_batch import IDENTITY_ENCODINGS, Q, expected, input_mix

pytestmark = pytest.mark.gpu
R_INV = pow(1 << 256, -1, Q)


@pytest.fixture(scope="module")
def lib():
    import halo2_prover_amd
    return halo2_prover_amd.load()


def c_verify_batch(L, params, items, idx, rng=None):
    """items: (proof, json) pairs -> (status, ok list, all_ok)"""
    n = len(items)
    proofs = (ctypes.c_char_p * n)(*[p for p, _ in items])
    lens = (ctypes.c_size_t * n)(*[len(p) for p, _ in items])
    jsons = (ctypes.c_char_p * n)(*[j.encode() for _, j in items])
    ok = (ctypes.c_int * n)(*([-1] * n))
    all_ok = ctypes.c_int(-1)
    rc = L.h2_verify_proofs(params, len(params), n, proofs, lens, jsons, idx, rng, None, ok, ctypes.byref(all_ok))
    return rc, list(ok), all_ok.value


def orbit(start):
    seq = [start]
    while seq[-1] != 1:
        seq.append(seq[-1] // 2 if seq[-1] % 2 == 0 else 3 * seq[-1] + 1)
    return seq


def simulate(L, js, idx):
    out = ctypes.create_string_buffer(256)
    n = ctypes.c_size_t(0)
    assert L.h2_simulate(js.encode(), idx, out, 256, ctypes.byref(n)) == 0
    return out.value.decode()


@pytest.fixture(scope="module")
def pools(h2, lib):
    """per circuit: (params, circuit index, 64 valid (proof, json) pairs -- the recorded proof first, then fresh ones made
    with OS randomness)"""
    rnd = random.Random(64)
    out = {}
    p4 = golden("params_k4.bin")
    items = [(golden("proof_arithmetic_k4.bin"), ARITH_INPUT)]
    while len(items) < 64:
        x, y, c = rnd.randrange(1 << 12), rnd.randrange(1 << 12), rnd.randrange(1 << 30)
        js = '{"x":%d,"y":%d,"constant":%d,"z":%d}' % (x, y, c, x * x * y * y + c)
        items.append((c_prove(lib, p4, js, 1, None), js))
    out["arithmetic"] = (p4, 1, items)
    p6 = golden("params_k6.bin")
    items = [(golden("proof_poseidon_k6.bin"), POSEIDON_INPUT)]
    while len(items) < 64:
        msg = (rnd.randrange(1 << 64), rnd.randrange(1 << 64))
        js = '{"x":[%d,%d],"output":"%s"}' % (msg[0], msg[1], simulate(lib, '{"x":[%d,%d]}' % msg, 2))
        items.append((c_prove(lib, p6, js, 2, None), js))
    out["poseidon"] = (p6, 2, items)
    p10 = c_setup(lib, 10, Stream(0))                      # the recorded Collatz proof was made under this SRS
    items = [(golden("proof_collatz_k10.bin"), COLLATZ_INPUT)]
    start = 2
    while len(items) < 64:
        start += 1
        seq = orbit(start)
        if len(seq) > 32:
            continue
        js = '{"x":%s}' % str(seq).replace(" ", "")
        items.append((c_prove(lib, p10, js, 0, None), js))
    out["collatz"] = (p10, 0, items)
    for name, (params, idx, its) in out.items():
        for at in (0, 1, len(its) - 1):
            assert c_verify(lib, params, its[at][0], its[at][1], idx) == (0, 1), (name, at, its[at][1])
    return out


def layout(name):
    """(offset of the first evaluation scalar, offset of the first byte behind the evaluations) of a proof, from the Python
    mirror's description of the circuit"""
    from halo2_prover_amd import prover
    circ = {"collatz": prover.CollatzCircuit([]), "arithmetic": prover.ArithmeticCircuit(1, 2, 3),
            "poseidon": prover.PoseidonCircuit([1, 2])}[name]
    pcols = len(circ.permutation_columns)
    chunk = circ.degree - 2
    sets = (pcols + chunk - 1) // chunk
    front = circ.num_advice + sets + 1 + (circ.degree - 1)
    evals = len(circ.advice_queries) + len(circ.fixed_queries) + 1 + pcols + (3 * sets - 1 if sets else 0)
    return 32 * front, 32 * (front + evals)


# ------------------------------------------------------------------------------------- the decompression kernel ----
def device_decompress(L, words, stream=None, curve=0):
    import torch
    n = len(words)
    d_in = torch.frombuffer(bytearray(b"".join(words)), dtype=torch.uint8).cuda()
    d_out = torch.full((64 * n,), 0xAB, dtype=torch.uint8, device="cuda")
    d_st = torch.full((n,), 0xCD, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc = L.h2_points_decompress_device(curve, d_in.data_ptr(), n, d_out.data_ptr(), d_st.data_ptr(),
                                       stream.cuda_stream if stream is not None else None)
    if rc != 0:
        return rc, None
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    raw, st = bytes(d_out.cpu().numpy()), bytes(d_st.cpu().numpy())
    pts = [(int.from_bytes(raw[64 * i:64 * i + 32], "little") * R_INV % Q,
            int.from_bytes(raw[64 * i + 32:64 * i + 64], "little") * R_INV % Q, st[i]) for i in range(n)]
    for i in range(n):       # the output is canonical Montgomery form, not merely congruent
        assert int.from_bytes(raw[64 * i:64 * i + 32], "little") < Q and int.from_bytes(raw[64 * i + 32:64 * i + 64], "little") < Q
    return 0, pts


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000, 40000])
def test_decompression_kernel_matches_big_integers(h2, lib, n):
    import torch
    words = input_mix(n, 77 + n)
    want = [expected(w) for w in words]
    rc, got = device_decompress(lib, words)
    assert rc == 0
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, words[i].hex(), g, w)
    rc, again = device_decompress(lib, words, stream=torch.cuda.Stream())
    assert rc == 0 and again == got
    if n >= 1000:
        assert {w[2] for w in want} == {0, 1, 2, 3}


def test_decompression_is_bn254_only_and_checks_its_arguments(h2, lib):
    import torch
    assert device_decompress(lib, input_mix(4, 1), curve=1) == (-1, None)             # H2_PALLAS
    assert device_decompress(lib, input_mix(4, 1), curve=2) == (-1, None)
    buf = torch.zeros(256, dtype=torch.uint8, device="cuda")
    assert lib.h2_points_decompress_device(0, None, 1, buf.data_ptr(), buf.data_ptr(), None) == -1
    assert lib.h2_points_decompress_device(0, buf.data_ptr() + 4, 1, buf.data_ptr() + 64, buf.data_ptr() + 128, None) == -1
    assert lib.h2_points_decompress_device(0, None, 0, None, None, None) == 0


# ------------------------------------------------------------------------------------------ batches of valid proofs ----
@pytest.mark.parametrize("name", ["arithmetic", "poseidon", "collatz"])
@pytest.mark.parametrize("n", [1, 2, 17, 64])
def test_batches_of_valid_proofs_take_one_pairing(h2, lib, pools, name, n):
    params, idx, items = pools[name]
    before = lib.h2_selftest_pairing_checks()
    rc, ok, all_ok = c_verify_batch(lib, params, items[:n], idx)
    assert (rc, ok, all_ok) == (0, [1] * n, 1)
    assert lib.h2_selftest_pairing_checks() - before == 1
    before = lib.h2_selftest_pairing_checks()
    assert c_verify(lib, params, items[0][0], items[0][1], idx) == (0, 1)
    assert lib.h2_selftest_pairing_checks() - before == 1                 # the single verifier counts too


def test_python_wrapper(h2, lib, pools):
    params, idx, items = pools["poseidon"]
    bad = bytearray(items[2][0])
    bad[40] ^= 4
    proofs = [p for p, _ in items[:5]]
    proofs[2] = bytes(bad)
    assert h2.verify_proofs(params, proofs, [j for _, j in items[:5]], idx) == [True, True, False, True, True]
    assert h2.verify_proofs(params, [], [], idx) == []
    assert h2.verify_proofs(params, proofs[:2], [j for _, j in items[:2]], idx, rng=lambda k: bytes(range(k))) == [True, True]


# --------------------------------------------------------------------------------- agreement with the single verifier ----
def corruptions(name, pools):
    """(label, proof, json) replacements for a good item of circuit `name`"""
    params, idx, items = pools[name]
    proof, js = items[5]
    scalar_at, opening_at = layout(name)
    assert opening_at < len(proof) and (len(proof) - opening_at) % 32 == 0

    def flip(at, bit=2):
        b = bytearray(proof)
        b[at] ^= bit
        return bytes(b)
    out = [("bit in a commitment", flip(7), js), ("bit in the second commitment", flip(33), js),
           ("bit in an evaluation", flip(scalar_at + 3), js), ("bit in the last evaluation", flip(opening_at - 30), js),
           ("bit in an opening point", flip(len(proof) - 20), js), ("bit in the first opening point", flip(opening_at + 1), js)]
    for i, enc in enumerate(IDENTITY_ENCODINGS):
        out.append(("identity commitment, encoding %d" % i, enc + proof[32:], js))
        out.append(("identity opening, encoding %d" % i, proof[:-32] + enc, js))
    out += [("truncated", proof[:-32], js), ("truncated inside the commitments", proof[:40], js), ("empty", b"", js),
            ("32 extra bytes", proof + bytes(range(32)), js)]
    other = "poseidon" if name != "poseidon" else "arithmetic"
    out.append(("another circuit's proof", pools[other][2][1][0], js))
    if name == "arithmetic":
        x, y, c, z = [int(v.split(":")[1]) for v in js.strip("{}").split(",")]
        out.append(("public input off by one", proof, '{"x":%d,"y":%d,"constant":%d,"z":%d}' % (x, y, c, z + 1)))
    elif name == "poseidon":
        out.append(("a false claim", proof, items[6][1]))                 # another message's input
    else:
        out.append(("another orbit's input", proof, items[6][1]))         # Collatz has no public input: still valid
    return out


@pytest.mark.parametrize("name", ["arithmetic", "poseidon", "collatz"])
def test_batch_agrees_with_the_single_verifier_item_by_item(h2, lib, pools, name):
    params, idx, items = pools[name]
    base = items[16:32]
    cases = corruptions(name, pools)
    singles = {label: c_verify(lib, params, proof, js, idx) for label, proof, js in cases}
    assert len(singles) == len(cases)
    assert all(rc == 0 for rc, _ in singles.values())
    rejected = [label for label, (_, ok) in singles.items() if ok == 0]
    assert len(rejected) >= len(cases) - 2, singles            # extra bytes (and Collatz's unused input) are accepted
    for label, proof, js in cases:
        for places in ((3,), (4,), (11,), (3, 4, 11)):
            batch = list(base)
            for at in places:
                batch[at] = (proof, js)
            want = [singles[label][1] if i in places else 1 for i in range(16)]
            rc, ok, all_ok = c_verify_batch(lib, params, batch, idx)
            assert (rc, ok, all_ok) == (0, want, int(all(want))), (label, places)
    # all of them in one batch, between good neighbours
    batch, want = [], []
    for label, proof, js in cases:
        batch += [(proof, js), base[len(batch) % 16]]
        want += [singles[label][1], 1]
    assert c_verify_batch(lib, params, batch, idx) == (0, want, 0)


# ---------------------------------------------------------------------------------------------------------- weights ----
def test_weights_come_from_the_callers_rng(h2, lib, pools):
    from halo2_prover_amd import lib as h2lib
    params, idx, items = pools["arithmetic"]
    bad = (items[1][0][:64] + bytes([items[1][0][64] ^ 1]) + items[1][0][65:], items[1][1])
    assert c_verify(lib, params, bad[0], bad[1], idx) == (0, 0)
    asked = []

    def counting(_ctx, out, n):
        asked.append(n)
        data = random.Random(len(asked)).randbytes(n)
        ctypes.memmove(out, data, n)
    for n in (2, 17):
        del asked[:]
        assert c_verify_batch(lib, params, items[:n], idx, h2lib.RNG_FILL(counting))[1] == [1] * n
        assert sum(asked) >= 16 * (n - 1)

    def zeros(_ctx, out, n):
        ctypes.memset(out, 0, n)
    zero_cb = h2lib.RNG_FILL(zeros)
    assert c_verify_batch(lib, params, [items[0], bad], idx, zero_cb) == (0, [1, 0], 0)
    assert c_verify_batch(lib, params, [bad, items[0]], idx, zero_cb) == (0, [0, 1], 0)
    assert c_verify_batch(lib, params, items[:8], idx, zero_cb) == (0, [1] * 8, 1)

    def fixed_stream():
        state = random.Random(99)

        def fill(_ctx, out, n):
            ctypes.memmove(out, state.randbytes(n), n)
        return h2lib.RNG_FILL(fill)
    batch = items[:6] + [bad] + items[6:10]
    first = c_verify_batch(lib, params, batch, idx, fixed_stream())
    assert first == c_verify_batch(lib, params, batch, idx, fixed_stream())
    assert first == (0, [1] * 6 + [0] + [1] * 4, 0)


# -------------------------------------------------------------------------------------------------------- bisection ----
@pytest.mark.parametrize("name", ["arithmetic", "collatz"])
def test_one_bad_proof_among_64_is_found_by_halving(h2, lib, pools, name):
    params, idx, items = pools[name]
    rnd = random.Random()
    at = rnd.randrange(64)
    proof = bytearray(items[at][0])
    proof[len(proof) - 5] ^= 0x10                       # an opening point: the replay may pass, the pairing cannot
    batch = list(items)
    batch[at] = (bytes(proof), items[at][1])
    before = lib.h2_selftest_pairing_checks()
    rc, ok, all_ok = c_verify_batch(lib, params, batch, idx)
    used = lib.h2_selftest_pairing_checks() - before
    assert (rc, ok, all_ok) == (0, [int(i != at) for i in range(64)], 0), at
    assert used <= 1 + 2 * int(math.log2(64)), (at, used)
    # a proof that fails in the replay never enters a combination
    batch[at] = (b"", items[at][1])
    before = lib.h2_selftest_pairing_checks()
    assert c_verify_batch(lib, params, batch, idx)[1] == [int(i != at) for i in range(64)]
    assert lib.h2_selftest_pairing_checks() - before == 1


# ----------------------------------------------------------------------------------------------------- status codes ----
def test_status_codes(h2, lib, pools):
    params, idx, items = pools["arithmetic"]
    all_ok = ctypes.c_int(-1)
    assert lib.h2_verify_proofs(params, len(params), 0, None, None, None, idx, None, None, None, ctypes.byref(all_ok)) == 0
    assert all_ok.value == 1
    n = 2
    proofs = (ctypes.c_char_p * n)(*[p for p, _ in items[:n]])
    lens = (ctypes.c_size_t * n)(*[len(p) for p, _ in items[:n]])
    jsons = (ctypes.c_char_p * n)(*[j.encode() for _, j in items[:n]])
    ok = (ctypes.c_int * n)(-1, -1)
    assert lib.h2_verify_proofs(params, len(params), n, proofs, lens, jsons, idx, None, None, None, ctypes.byref(all_ok)) == -1
    assert lib.h2_verify_proofs(params, len(params), n, None, lens, jsons, idx, None, None, ok, ctypes.byref(all_ok)) == -1
    assert all_ok.value == 0
    assert lib.h2_verify_proofs(params, len(params), n, proofs, lens, jsons, idx, None, None, ok, None) == 0   # all_ok is optional
    assert list(ok) == [1, 1]
    rc, ok, all_ok = c_verify_batch(lib, params, [items[0], (items[1][0], "{"), items[2]], idx)
    assert (rc, ok, all_ok) == (-6, [0, 0, 0], 0)                        # malformed JSON in one item: H2_EPROOF
    assert c_verify_batch(lib, params[:100], items[:2], idx)[0] == -6    # malformed params
    # a params blob from another setup of a sufficient k: nothing verifies, as with the single call
    p8 = c_setup(lib, 8, None)
    assert c_verify(lib, p8, items[0][0], items[0][1], idx) == (0, 0)
    assert c_verify_batch(lib, p8, items[:3], idx) == (0, [0, 0, 0], 0)


# ------------------------------------------------------------------------------------------------------- bystanders ----
def test_caches_change_nothing(h2, lib, pools):
    params, idx, items = pools["poseidon"]
    bad = bytearray(items[3][0])
    bad[100] ^= 1
    batch = items[:3] + [(bytes(bad), items[3][1])] + items[4:9]
    want = (0, [1, 1, 1, 0, 1, 1, 1, 1, 1], 0)
    assert c_verify_batch(lib, params, batch, idx) == want
    assert lib.h2_params_cache_clear() == 0
    assert c_verify_batch(lib, params, batch, idx) == want
    old = lib.h2_key_cache(0)
    try:
        assert c_verify_batch(lib, params, batch, idx) == want
        assert c_verify_batch(lib, params, batch, idx) == want
        assert c_verify(lib, params, items[0][0], items[0][1], idx) == (0, 1)
    finally:
        lib.h2_key_cache(old)
    assert c_verify_batch(lib, params, batch, idx) == want
