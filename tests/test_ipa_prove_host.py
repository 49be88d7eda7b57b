"""CPU (no GPU): the pieces of the IPA prover's transcript step (csrc/h2_ipa_prove.hpp) through their host instantiation --
the inversion by a fixed number of divsteps against pow(x, -1, p) on every field, and one lane's byte work behind a round
and behind the final kernel against transcript.Blake2bMidstate and transcript.compress, from midstates whose block buffer
stands at every place where the 131 absorbed bytes straddle the ring differently."""
import ctypes
import random

import pytest

from halo2_prover_amd.transcript import FIELDS, Blake2bMidstate, compress

H2_OK, H2_EINVAL = 0, -1
# h2_selftest_field_op's numbering: bn254 Fq, bn254 Fr, pasta Fp, pasta Fq
PRIMES = {0: FIELDS[0][1], 1: FIELDS[0][0], 2: FIELDS[2][0], 3: FIELDS[1][0]}
CID = {"pallas": 1, "vesta": 2}
BUFLENS = [0, 1, 62, 63, 126, 127, 128]


def L():
    from halo2_prover_amd import lib
    return lib.load()


def limbs(v):
    return (ctypes.c_uint64 * 4)(*[(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)])


def value(arr, at=0):
    return sum(int(arr[at + i]) << (64 * i) for i in range(4))


def mont(v, p):
    return v % p * ((1 << 256) % p) % p


def unmont(v, p):
    return v * pow(1 << 256, -1, p) % p


@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("field", [0, 1, 2, 3])
def test_the_inversion_is_the_canonical_inverse(field, form):
    """0, 1, 2, p - 1, p - 2 and 200 random values: 1 / x as pow gives it, and 0 for 0; form 1 is fe_inv, the baseline"""
    p = PRIMES[field]
    rnd = random.Random(0x1A7 + field)
    xs = [0, 1, 2, p - 1, p - 2] + [rnd.randrange(p) for _ in range(200)]
    out = (ctypes.c_uint64 * 4)()
    for x in xs:
        assert L().h2_selftest_field_inv(field, form, limbs(mont(x, p)), out) == H2_OK
        got = value(out)
        assert got < p, "the result is canonical"
        assert unmont(got, p) == (pow(x, -1, p) if x else 0), "1 / %d" % x


def test_the_inversion_hook_refuses_what_it_does_not_know():
    out = (ctypes.c_uint64 * 4)()
    assert L().h2_selftest_field_inv(4, 0, limbs(1), out) == H2_EINVAL
    assert L().h2_selftest_field_inv(2, 2, limbs(1), out) == H2_EINVAL
    assert L().h2_selftest_field_inv(2, 0, None, out) == H2_EINVAL


def midstate(curve, buflen, compressed_blocks):
    """a transcript with 128 * compressed_blocks + buflen bytes absorbed: the buffer holds buflen of them (a full buffer
    stays uncompressed until more input follows)"""
    m = Blake2bMidstate(curve)
    total = 128 * compressed_blocks + buflen
    if total:
        m.update(bytes((7 * i + 3) & 0xFF for i in range(total)))
    st = m.export()
    if buflen or compressed_blocks == 0:
        assert int.from_bytes(st[200:204], "little") == buflen
    return m


def points(curve, rnd, shape):
    """L, R as (x, y) or None; shape: y's parity per point, or None for the identity"""
    q = FIELDS[CID[curve]][1]
    out = []
    for par in shape:
        if par is None:
            out.append(None)
        else:
            out.append((rnd.randrange(q), 2 * rnd.randrange(q // 2) + par))
    return out


SHAPES = [(0, 1), (1, 0), (None, 1), (0, None), (None, None)]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("buflen", BUFLENS)
@pytest.mark.parametrize("curve", ["pallas", "vesta"])
def test_a_lanes_round_against_the_host_transcript(curve, buflen, shape):
    cid = CID[curve]
    p, q = FIELDS[cid][:2]
    rnd = random.Random(0xB17E + 131 * buflen + cid)
    for blocks in (0, 2):
        if blocks and buflen == 0:
            continue                                     # 256 bytes absorbed stand as one compressed block and a full buffer
        want = midstate(curve, buflen, blocks)
        state_in = want.export()
        lp, rp = points(curve, rnd, shape)
        lr = (ctypes.c_uint64 * 16)()
        for i, pt in enumerate((lp, rp)):
            x, y = pt if pt is not None else (0, 0)
            for w, c in enumerate((x, y)):
                lr[8 * i + 4 * w:8 * i + 4 * w + 4] = list(limbs(mont(c, q)))
        l, r, f = rnd.randrange(p), rnd.randrange(p), rnd.randrange(p)
        lrf = (ctypes.c_uint64 * 12)(*(list(limbs(mont(l, p))) + list(limbs(mont(r, p))) + list(limbs(mont(f, p)))))
        wire, state_out = ctypes.create_string_buffer(64), ctypes.create_string_buffer(208)
        out, status = (ctypes.c_uint64 * 12)(), ctypes.c_uint32(7)
        assert L().h2_selftest_ipa_step(cid, 0, state_in, lr, lrf, wire, state_out, out, ctypes.byref(status)) == H2_OK
        want.common_point(lp)
        want.common_point(rp)
        u = want.squeeze_challenge()
        assert wire.raw == compress(cid, lp) + compress(cid, rp)
        assert unmont(value(out, 0), p) == u
        assert unmont(value(out, 4), p) == pow(u, -1, p)
        assert unmont(value(out, 8), p) == (f + l * pow(u, -1, p) + r * u) % p
        assert status.value == 0
        assert state_out.raw == want.export()


@pytest.mark.parametrize("buflen", BUFLENS)
@pytest.mark.parametrize("curve", ["pallas", "vesta"])
def test_a_lanes_scalars_against_the_host_transcript(curve, buflen):
    """c and f behind the final kernel: 32 canonical bytes to the proof, 0x02 and those bytes absorbed"""
    cid = CID[curve]
    p = FIELDS[cid][0]
    rnd = random.Random(0x5CA1 + buflen + cid)
    want = midstate(curve, buflen, 1 if buflen else 0)
    state = want.export()
    for s in (rnd.randrange(p), 0, p - 1):
        canon, state_out = ctypes.create_string_buffer(32), ctypes.create_string_buffer(208)
        assert L().h2_selftest_ipa_step_scalar(cid, state, limbs(mont(s, p)), canon, state_out) == H2_OK
        want.common_scalar(s)
        assert canon.raw == s.to_bytes(32, "little")
        assert state_out.raw == want.export()
        state = state_out.raw


@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("curve", ["pallas", "vesta"])
def test_a_zero_challenge_is_flagged_and_divides_nothing(curve, form):
    cid = CID[curve]
    p = FIELDS[cid][0]
    l, r, f = 5, 7, 11
    out, status = (ctypes.c_uint64 * 8)(), ctypes.c_uint32(7)
    for u in (0, 3):
        vin = (ctypes.c_uint64 * 16)(*[w for v in (u, l, r, f) for w in limbs(mont(v, p))])
        assert L().h2_selftest_ipa_fold(cid, form, vin, out, ctypes.byref(status)) == H2_OK
        ui = pow(u, -1, p) if u else 0
        assert unmont(value(out, 0), p) == ui
        assert unmont(value(out, 4), p) == (f + l * ui + r * u) % p
        assert status.value == (0 if u else 1)
    assert L().h2_selftest_ipa_fold(0, form, vin, out, ctypes.byref(status)) == H2_EINVAL     # BN254: not this wire form
