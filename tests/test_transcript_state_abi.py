"""The transcript midstate of the C ABI (h2_transcript_state_t, h2_transcript_init / _absorb / _challenge) against hashlib,
and transcript.Blake2bMidstate against Blake2bTranscript.  Host only: no device, no h2_init."""
import ctypes
import hashlib
import random

import pytest

from halo2_prover_amd import lib as _lib
from halo2_prover_amd.transcript import FIELDS, STATE_BYTES, Blake2bMidstate, Blake2bTranscript

# absorbed lengths around the block size: an empty buffer, a full uncompressed one (128, 256), one byte into the next block
LENGTHS = [0, 1, 63, 64, 127, 128, 129, 255, 256, 257, 1000]
PIECES = [None, 1, 33, 65]                          # None: in one piece


class State(ctypes.Structure):
    _fields_ = [("h", ctypes.c_uint64 * 8), ("t", ctypes.c_uint64), ("buf", ctypes.c_uint8 * 128), ("buflen", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32)]


def data(n, seed=0):
    return bytes(random.Random(0x54525343 + seed).getrandbits(8) for _ in range(n))


def absorb(L, st, blob, piece):
    step = piece or max(1, len(blob))
    for at in range(0, len(blob), step):
        part = blob[at:at + step]
        assert L.h2_transcript_absorb(ctypes.byref(st), part, len(part)) == 0


def challenge(L, curve, st):
    out = (ctypes.c_uint64 * 4)()
    assert L.h2_transcript_challenge(curve, ctypes.byref(st), out) == 0
    p = FIELDS[curve][0]
    return sum(int(out[i]) << (64 * i) for i in range(4)) * pow(1 << 256, -1, p) % p


def test_struct_is_208_bytes():
    assert ctypes.sizeof(State) == 208 == STATE_BYTES
    assert (State.h.offset, State.t.offset, State.buf.offset, State.buflen.offset, State.reserved.offset) == (0, 64, 72, 200, 204)
    assert len(Blake2bMidstate("pallas").export()) == 208


@pytest.mark.parametrize("piece", PIECES)
@pytest.mark.parametrize("length", LENGTHS)
def test_midstate_against_hashlib(length, piece):
    L = _lib.load()
    blob, more = data(length), data(77, seed=1)
    for curve in (0, 1, 2):
        p = FIELDS[curve][0]
        st = State()
        assert L.h2_transcript_init(ctypes.byref(st)) == 0
        absorb(L, st, blob, piece)
        assert st.buflen == (length if length <= 128 else (length - 1) % 128 + 1) and st.t == length - st.buflen
        ref = hashlib.blake2b(digest_size=64, person=b"Halo2-Transcript")
        ref.update(blob + b"\x00")
        assert challenge(L, curve, st) == int.from_bytes(ref.copy().digest(), "little") % p, (curve, length, piece)
        # the copy was finalised, not the state: it keeps absorbing
        absorb(L, st, more, piece)
        ref.update(more + b"\x00")
        assert challenge(L, curve, st) == int.from_bytes(ref.digest(), "little") % p, (curve, length, piece)
        assert st.reserved == 0 and not any(st.buf[st.buflen:])           # the bytes behind buflen are zero: one form per state


@pytest.mark.parametrize("curve", ["bn254", "pallas", "vesta"])
def test_wrapper_against_blake2b_transcript(curve):
    rnd = random.Random(0x4D494453)
    ref, mid = Blake2bTranscript(curve), Blake2bMidstate(curve)
    p, q = ref.p, ref.q
    assert (mid.p, mid.q) == (p, q)

    def step(a, b, i):
        kind = i % 4
        if kind == 0:
            pt = (rnd.randrange(q), rnd.randrange(q)) if i % 12 else None       # the transcript does not ask for a curve point
            a.common_point(pt)
            b.common_point(pt)
        elif kind == 1:
            s = rnd.randrange(p)
            a.common_scalar(s)
            b.common_scalar(s)
        elif kind == 2:
            blob = data(rnd.randrange(0, 200), seed=i)
            a.state.update(blob)
            b.update(blob)
        else:
            assert a.squeeze_challenge() == b.squeeze_challenge(), i
    for i in range(40):
        step(ref, mid, i)
    # the export fed to a fresh state continues identically, and leaves the exporter alone
    exported = mid.export()
    again = Blake2bMidstate(curve, state=exported)
    assert again.export() == exported == mid.export()
    for i in range(40, 60):
        step(ref, again, i)
    assert mid.export() == exported
    with pytest.raises(ValueError):
        Blake2bMidstate(curve, state=exported[:-1])


def test_argument_checks():
    L = _lib.load()
    st = State()
    out = (ctypes.c_uint64 * 4)()
    assert L.h2_transcript_init(None) == -1
    assert L.h2_transcript_init(ctypes.byref(st)) == 0
    assert L.h2_transcript_absorb(None, b"x", 1) == -1
    assert L.h2_transcript_absorb(ctypes.byref(st), None, 1) == -1
    assert L.h2_transcript_absorb(ctypes.byref(st), None, 0) == 0          # nothing to read
    assert L.h2_transcript_challenge(3, ctypes.byref(st), out) == -1        # unknown curve
    assert L.h2_transcript_challenge(1, None, out) == -1
    assert L.h2_transcript_challenge(1, ctypes.byref(st), None) == -1
    before = bytes(st)
    st.buflen = 129                                                         # not a state
    assert L.h2_transcript_absorb(ctypes.byref(st), b"x", 1) == -1
    assert L.h2_transcript_challenge(1, ctypes.byref(st), out) == -1
    st.buflen = 0
    assert bytes(st) == before                                              # a refused call leaves the state alone
