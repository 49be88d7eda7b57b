"""GPU: h2_ipa_create_proofs / ipa.create_proofs_bytes and h2_ipa_prove_rounds_device -- the IPA prover with the transcripts
on the device.

The judge of the bytes is ipa.create_proofs, the host loop this route does not touch: the same polynomials, points, blinds,
s_poly and rng seeds must give the same proof byte for byte, and leave the transcript where a host transcript that absorbed
that proof stands.  The rounds alone are held against h2_ipa_*_batch_device driven by a Python loop; the proofs against
ipa.verify_proofs_bytes and test_gpu_ipa_proof.py's host verifier, which makes no GPU call."""
import ctypes
import random

import numpy as np
import pytest

import test_gpu_ipa as T
import test_gpu_ipa_batch as TB
import test_gpu_ipa_proof as TP

pytestmark = pytest.mark.gpu

H2_OK, H2_EINVAL, H2_EHANDLE = 0, -1, -4
CURVES = ["pallas", "vesta"]
CID = TP.CID

_PARAMS = {}


def params_of(curve, k):
    """ParamsIPA of one (curve, k) and the points it registered, made once"""
    key = (curve, k)
    if key not in _PARAMS:
        import halo2_prover_amd as h2
        import oracle_lib as O
        from halo2_prover_amd import ipa
        h2.init(0)
        n = 1 << k
        pts = O.synth_bases(CID[curve], 0x49504300 + 16 * k + CID[curve], n + 2).reshape(n + 2, 8)
        _PARAMS[key] = (ipa.ParamsIPA(curve, k, pts[:n], pts[n + 1], pts[n]), pts)
    return _PARAMS[key]


def specs(curve, k, m, seed, prefixes=None, seeded=()):
    """m openings: polynomial, blind, x3, s_poly (None for the indices in `seeded`), the rng's seed, the transcript's prefix"""
    params, _ = params_of(curve, k)
    p, n = params.p, 1 << k
    R = (1 << 256) % p
    rnd = random.Random(seed)
    out = []
    for i in range(m):
        poly = [rnd.randrange(p) for _ in range(n)]
        if i == 1:
            poly = [0] * n                                # a zero polynomial among them
        s_poly = [rnd.randrange(p) for _ in range(n)]
        out.append(dict(poly=poly, poly_m=TP.limbs([c * R % p for c in poly]), blind=rnd.randrange(p), x3=rnd.randrange(1, p),
                        s_m=None if i in seeded else TP.limbs([c * R % p for c in s_poly]), rng=seed * 1000 + i,
                        prefix=bytes(rnd.getrandbits(8) for _ in range(prefixes[i] if prefixes else 0))))
    return out


def host_proofs(curve, k, S):
    """ipa.create_proofs, the yardstick -> (proofs, nothing else: hashlib's state cannot be exported)"""
    import halo2_prover_amd as h2
    from halo2_prover_amd import ipa
    params, _ = params_of(curve, k)
    items = []
    for s in S:
        tr = h2.Blake2bTranscript(curve)
        tr.state.update(s["prefix"])
        items.append((tr, s["poly_m"], s["blind"], s["x3"], TP.Rng(s["rng"]), s["s_m"]))
    return ipa.create_proofs(params, items)


def device_proofs(curve, k, S):
    """ipa.create_proofs_bytes on the same openings -> (proofs, the midstates afterwards)"""
    from halo2_prover_amd import ipa
    from halo2_prover_amd.transcript import Blake2bMidstate
    params, _ = params_of(curve, k)
    mids = []
    for s in S:
        mids.append(Blake2bMidstate(curve))
        mids[-1].update(s["prefix"])
    items = [(mids[i], s["poly_m"], s["blind"], s["x3"], TP.Rng(s["rng"]), s["s_m"]) for i, s in enumerate(S)]
    return ipa.create_proofs_bytes(params, items), [m.export() for m in mids]


def absorbed(curve, k, prefix, proof):
    """the midstate of a host transcript that absorbed `prefix` and read `proof` as verify_proof reads it"""
    from halo2_prover_amd.transcript import Blake2bMidstate, decompress
    cid = CID[curve]
    mid = Blake2bMidstate(curve)
    mid.update(prefix)
    chunks = [proof[i:i + 32] for i in range(0, len(proof), 32)]
    assert len(chunks) == 2 * k + 3
    mid.common_point(decompress(cid, chunks[0]))
    mid.squeeze_challenge()
    mid.squeeze_challenge()
    for j in range(k):
        mid.common_point(decompress(cid, chunks[1 + 2 * j]))
        mid.common_point(decompress(cid, chunks[2 + 2 * j]))
        mid.squeeze_challenge()
    mid.common_scalar(int.from_bytes(chunks[2 * k + 1], "little"))
    mid.common_scalar(int.from_bytes(chunks[2 * k + 2], "little"))
    return mid.export()


def parity(curve, k, S):
    want = host_proofs(curve, k, S)
    got, mids = device_proofs(curve, k, S)
    assert len(got) == len(want) == len(S)
    for i, s in enumerate(S):
        assert len(got[i]) == 32 * (2 * k + 3)
        assert got[i] == want[i], "opening %d: the proof differs from ipa.create_proofs'" % i
        assert mids[i] == absorbed(curve, k, s["prefix"], want[i]), "opening %d: the midstate behind f" % i
    return got


SHAPES = [(k, m) for k in (1, 2, 3, 5) for m in (1, 2, 3)] + [(2, 64)]


@pytest.mark.parametrize("k,m", SHAPES)
@pytest.mark.parametrize("curve", CURVES)
def test_the_bytes_are_create_proofs_bytes(curve, k, m):
    parity(curve, k, specs(curve, k, m, 0xC0DE + 64 * k + m))


@pytest.mark.parametrize("curve", CURVES)
def test_s_poly_from_seeds_and_given_in_one_batch(curve):
    k = 3
    parity(curve, k, specs(curve, k, 4, 0x5EED, seeded=(0, 2)))
    parity(curve, k, specs(curve, k, 2, 0x5EEE, seeded=(0, 1)))      # no s_poly at all


@pytest.mark.parametrize("curve", CURVES)
def test_midstates_that_stand_at_different_places_of_the_block(curve):
    """lanes compress at different moments: 0, 63, 127, 128 bytes absorbed before S (and one past a block)"""
    k = 2
    parity(curve, k, specs(curve, k, 5, 0xB0F, prefixes=[0, 63, 127, 128, 200]))


@pytest.mark.parametrize("curve", CURVES)
def test_the_proofs_verify_and_a_flipped_byte_does_not(curve):
    from halo2_prover_amd import ipa
    from halo2_prover_amd.transcript import Blake2bMidstate
    k, m = 3, 3
    params, pts = params_of(curve, k)
    p = params.p
    S = specs(curve, k, m, 0x7E57)
    proofs, _ = device_proofs(curve, k, S)
    cases = []
    for s in S:
        v = sum(c * pow(s["x3"], i, p) for i, c in enumerate(s["poly"])) % p
        cases.append(dict(curve=curve, k=k, params=params, pts=pts, x3=s["x3"], v=v, P=params.commit(s["poly_m"], s["blind"])))
    for C, proof in zip(cases, proofs):
        assert TP.host_verify(C, proof, C["v"]), "the verifier that makes no GPU call"
        assert not TP.host_verify(C, TP.flip(proof, 32 * (1 + 2 * k) + 1), C["v"])          # c
        assert not TP.host_verify(C, proof, (C["v"] + 1) % p)
    bad = TP.flip(proofs[1], 32 * 2 + 5, 3)                                                # an R_0
    items = [(Blake2bMidstate(curve), pr, C["P"], C["x3"], C["v"]) for C, pr in zip(cases, [proofs[0], bad, proofs[2]])]
    assert ipa.verify_proofs_bytes(params, items, rng=TP.Rng(3)) == [True, False, True]
    items = [(Blake2bMidstate(curve), pr, C["P"], C["x3"], C["v"]) for C, pr in zip(cases, proofs)]
    assert ipa.verify_proofs_bytes(params, items, rng=TP.Rng(4)) == [True] * m


# ---- the rounds alone ----------------------------------------------------------------------------------------------------
def prove_state_bytes(k, m):
    need = ctypes.c_size_t(0)
    assert T.L().h2_ipa_prove_state_bytes(k, m, ctypes.byref(need)) == H2_OK
    return need.value


def rounds_reference(curve, k, ins, prefixes):
    """h2_ipa_*_batch_device driven from Python with a host transcript per opening -> (tails, midstates behind f)"""
    from halo2_prover_amd.transcript import Blake2bMidstate, compress
    cid = CID[curve]
    p, q = T.primes(curve)
    params, _ = params_of(curve, k)
    m = len(ins)
    B = TB.Batch(curve, k, m)
    mids = []
    for pre in prefixes:
        mids.append(Blake2bMidstate(curve))
        mids[-1].update(pre)
    start = [x.export() for x in mids]
    run = [dict(I, us=[]) for I in ins]
    f = [I["f0"] for I in ins]
    tails = [b"" for _ in ins]
    assert B.begin(run) == H2_OK
    for j in range(k):
        assert B.round(run, j) == H2_OK
        lr = T.from_dev(B.out)[:m].copy()
        for i, I in enumerate(run):
            for half in (lr[i, :8], lr[i, 8:]):
                pt = params.affine_ints(half)
                mids[i].common_point(pt)
                tails[i] += compress(cid, pt)
            u = mids[i].squeeze_challenge()
            I["us"].append(u)
            l_j, r_j = I["blinds"][j]
            f[i] = (f[i] + l_j * pow(u, -1, p) + r_j * u) % p
    assert B.final(run) == H2_OK
    cb = T.from_dev(B.out).reshape(-1)[:8 * m].reshape(m, 8)
    rinv = pow(1 << 256, -1, p)
    for i in range(m):
        c = int.from_bytes(cb[i, :4].tobytes(), "little") * rinv % p
        for s in (c, f[i]):
            mids[i].common_scalar(s)
            tails[i] += s.to_bytes(32, "little")
    return start, tails, [x.export() for x in mids]


def rounds_device(curve, k, ins, start, state, handle=None, tweak=None):
    """h2_ipa_prove_rounds_device on the caller's state tensor -> (status code, tails, midstates, status words); tweak(arrays)
    edits the scalar arrays (x3, z, f0: m rows; blinds: 2 k m rows) before the call"""
    import torch
    p, _ = T.primes(curve)
    m = len(ins)
    S = T.setup(curve, k)
    polys = [T.to_dev(T.mont(p, I["a"])) for I in ins]
    d_p = (ctypes.c_void_p * m)(*[t.data_ptr() for t in polys])
    x3, z, f0 = T.mont(p, [I["x3"] for I in ins]), T.mont(p, [I["z"] for I in ins]), T.mont(p, [I["f0"] for I in ins])
    blinds = T.mont(p, [b for I in ins for lr in I["blinds"] for b in lr])
    if tweak:
        tweak(dict(x3=x3, z=z, f0=f0, blinds=blinds))
    states = ctypes.create_string_buffer(b"".join(start), 208 * m)
    tail = torch.full((m * (2 * k + 2) * 4,), -1, dtype=torch.int64, device="cuda")
    mids = torch.full((m * 26,), -1, dtype=torch.int64, device="cuda")
    status = torch.full((m,), 9, dtype=torch.int32, device="cuda")
    rc = T.L().h2_ipa_prove_rounds_device(CID[curve], S["bases"].handle if handle is None else handle, k, m, d_p, x3.ctypes.data,
                                          z.ctypes.data, f0.ctypes.data, blinds.ctypes.data, states, ctypes.c_void_p(state.data_ptr()),
                                          ctypes.c_void_p(tail.data_ptr()), ctypes.c_void_p(mids.data_ptr()),
                                          ctypes.c_void_p(status.data_ptr()), None)
    raw = tail.cpu().numpy().tobytes()
    per = 32 * (2 * k + 2)
    mraw = mids.cpu().numpy().tobytes()
    return rc, [raw[i * per:(i + 1) * per] for i in range(m)], [mraw[208 * i:208 * (i + 1)] for i in range(m)], status.cpu().tolist()


def round_inputs(curve, k, m, seed):
    p, _ = T.primes(curve)
    rnd = random.Random(seed)
    ins = TB.openings(curve, k, m, seed)
    for I in ins:
        I["f0"] = rnd.randrange(p)
    return ins


@pytest.mark.parametrize("curve", CURVES)
def test_the_rounds_alone_against_the_python_loop(curve):
    """L_j || R_j of every round in the wire form, c, f, the midstate and a zero status -- on a fresh state, on the same
    state again after a use with another m, and on a state full of 0xFF bytes: what an earlier use left does not matter"""
    import torch
    k = 3
    state = torch.zeros(prove_state_bytes(k, 2) // 8, dtype=torch.int64, device="cuda")
    want = {}
    for m in (1, 2):
        ins = round_inputs(curve, k, m, 0xA110 + m)
        prefixes = [b"", b"x" * 100][:m]
        want[m] = (ins,) + rounds_reference(curve, k, ins, prefixes)
    for m in (2, 1, 2, "fill", 1, 2):
        if m == "fill":
            state.fill_(-1)
            continue
        ins, start, tails, mids = want[m]
        rc, got_tails, got_mids, status = rounds_device(curve, k, ins, start, state)
        assert rc == H2_OK
        assert status == [0] * m
        for i in range(m):
            assert got_tails[i] == tails[i], "m = %d, opening %d" % (m, i)
            assert got_mids[i] == mids[i]


@pytest.mark.parametrize("curve", CURVES)
def test_the_older_routes_are_what_they_were(curve):
    """one state driven by h2_ipa_begin_batch_device ... final before and after a h2_ipa_create_proofs call on the same
    context: the same bytes (m = 1 takes its scalars by value, m = 2 from the table, as before)"""
    k = 3
    for m in (1, 2):
        ins = TB.openings(curve, k, m, 0x01D + m)
        B = TB.Batch(curve, k, m)
        before = B.run(ins)
        device_proofs(curve, k, specs(curve, k, 2, 0x01E))
        after = B.run(ins)
        for a, b in zip(before[0], after[0]):
            assert np.array_equal(a, b)
        assert np.array_equal(before[1], after[1])


@pytest.mark.parametrize("curve", CURVES)
def test_the_arenas_are_released_and_taken_again(curve):
    """calls of different m in a row on one context: the same bytes each time, and the third allocates nothing"""
    k = 3
    wide, narrow = specs(curve, k, 3, 0xA4E), specs(curve, k, 1, 0xA4F)
    first, _ = device_proofs(curve, k, wide)
    one, _ = device_proofs(curve, k, narrow)
    stats = (ctypes.c_uint64 * 4)()
    assert T.L().h2_selftest_arena_stats(stats) == H2_OK
    grown = stats[0]
    again, _ = device_proofs(curve, k, wide)
    assert again == first
    assert device_proofs(curve, k, narrow)[0] == one
    assert T.L().h2_selftest_arena_stats(stats) == H2_OK
    assert stats[0] == grown


# ---- what is refused, before anything is enqueued ----------------------------------------------------------------------------
def create_raw(curve, k, S, cid=None, kk=None, mm=None, handle=None, seeds=True, tweak=None):
    """h2_ipa_create_proofs itself on the openings S -> (status code, the proofs buffer); tweak(args) edits the arguments"""
    from halo2_prover_amd.transcript import Blake2bMidstate
    params, _ = params_of(curve, k)
    p = params.p
    m = len(S)
    polys = [T.to_dev(s["poly_m"]) for s in S]
    s_polys = [None if s["s_m"] is None else T.to_dev(s["s_m"]) for s in S]
    args = dict(
        states=ctypes.create_string_buffer(b"".join(Blake2bMidstate(curve).export() for _ in S), 208 * m),
        d_p=(ctypes.c_void_p * m)(*[t.data_ptr() for t in polys]),
        p_blind=T.mont(p, [s["blind"] for s in S]), x3=T.mont(p, [s["x3"] for s in S]),
        d_s=(ctypes.c_void_p * m)(*[None if t is None else t.data_ptr() for t in s_polys]),
        seeds=ctypes.create_string_buffer(bytes(range(32)) * m, 32 * m) if seeds else None,
        s_blind=T.mont(p, [7 + i for i in range(m)]), blinds=T.mont(p, [11 + i for i in range(2 * k * m)]))
    if tweak:
        tweak(args)
    proofs = ctypes.create_string_buffer(b"\xA5" * (m * 32 * (2 * k + 3)), m * 32 * (2 * k + 3))
    status = (ctypes.c_uint32 * m)(*([9] * m))
    rc = T.L().h2_ipa_create_proofs(CID[curve] if cid is None else cid, params.bases.handle if handle is None else handle,
                                    k if kk is None else kk, m if mm is None else mm, args["states"], args["d_p"],
                                    args["p_blind"].ctypes.data, args["x3"].ctypes.data, args["d_s"], args["seeds"],
                                    args["s_blind"].ctypes.data, args["blinds"].ctypes.data, proofs, None, status)
    return rc, proofs.raw, list(status)


def test_what_create_proofs_refuses():
    import halo2_prover_amd as h2
    curve, k = "pallas", 2
    params, pts = params_of(curve, k)
    p = params.p
    S = specs(curve, k, 2, 0xBAD)
    untouched = b"\xA5" * (2 * 32 * (2 * k + 3))
    rc, raw, status = create_raw(curve, k, S)
    assert rc == H2_OK and raw != untouched and status == [0, 0]

    def refused(want=H2_EINVAL, **kw):
        rc, raw, status = create_raw(curve, k, S, **kw)
        assert rc == want
        assert raw == untouched and status == [9, 9], "nothing is written for a refused call"

    refused(cid=0)                                                   # BN254: the wire form is the Pasta one
    refused(cid=3)
    refused(kk=0)
    refused(kk=21)
    refused(mm=0)
    refused(mm=65)
    refused(want=H2_EHANDLE, handle=0xDEAD)
    short = h2.Bases(curve, pts[:(1 << k) + 1])                      # 2^k + 1 bases
    refused(handle=short.handle)
    params3, _ = params_of(curve, 3)
    refused(handle=params3.bases.handle)                             # the table of another k

    def ptr(name, i, value):
        def tweak(a):
            a[name][i] = value
        return tweak

    refused(tweak=ptr("d_p", 1, None))
    refused(tweak=lambda a: a["d_p"].__setitem__(0, a["d_p"][0] + 8))      # misaligned
    refused(tweak=lambda a: a["d_s"].__setitem__(1, a["d_s"][1] + 4))
    refused(tweak=ptr("d_s", 0, None), seeds=False)                  # a seed is needed and there are none

    def limb(name, row):
        def tweak(a):
            a[name][row] = TP.limbs([p])[0]                          # p itself: not canonical
        return tweak

    refused(tweak=limb("x3", 1))
    refused(tweak=limb("p_blind", 0))
    refused(tweak=limb("s_blind", 1))
    refused(tweak=limb("blinds", 2 * k * 2 - 1))

    def buflen(a):
        raw = bytearray(a["states"].raw)
        raw[208 + 200:208 + 204] = (129).to_bytes(4, "little")
        a["states"] = ctypes.create_string_buffer(bytes(raw), len(raw))

    refused(tweak=buflen)
    rc, raw, status = create_raw(curve, k, S, tweak=ptr("d_s", 0, None))   # with seeds: fine
    assert rc == H2_OK and status == [0, 0]


def test_what_the_rounds_call_refuses():
    import halo2_prover_amd as h2
    import torch
    curve, k, m = "vesta", 2, 2
    p, _ = T.primes(curve)
    ins = round_inputs(curve, k, m, 0xBAE)
    start, tails, mids = rounds_reference(curve, k, ins, [b"", b"y"])
    state = torch.zeros(prove_state_bytes(k, m) // 8 + 2, dtype=torch.int64, device="cuda")
    rc, got, _, status = rounds_device(curve, k, ins, start, state)
    assert rc == H2_OK and got == tails and status == [0, 0]
    untouched = b"\xFF" * (32 * (2 * k + 2))

    def refused(want=H2_EINVAL, ins=ins, start=start, st=state, **kw):
        rc, got, _, status = rounds_device(curve, k, ins, start, st, **kw)
        assert rc == want
        assert got == [untouched] * len(ins) and status == [9] * len(ins)

    refused(st=state[1:])                                            # d_state 8 bytes off
    refused(want=H2_EHANDLE, handle=0xDEAD)
    S = T.setup(curve, k)
    short = h2.Bases(curve, np.concatenate([S["g"], S["u"].reshape(1, 8)]))                   # 2^k + 1 bases
    refused(handle=short.handle)
    for name, row in (("x3", 1), ("z", 0), ("f0", 0), ("blinds", 2 * k * m - 1)):
        refused(tweak=lambda a, name=name, row=row: a[name].__setitem__(row, TP.limbs([p])[0]))      # p itself: not canonical
    raw = bytearray(start[0])
    raw[200:204] = (129).to_bytes(4, "little")
    refused(start=[bytes(raw), start[1]])
