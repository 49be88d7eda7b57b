"""halo2's Blake2b transcript with Challenge255 over the fields of any of the three curves.

Upstream (halo2_proofs @6b43b6b, src/transcript.rs -- un-vendored): a Blake2b state personalised
"Halo2-Transcript"; a scalar is absorbed as 0x02 and its 32 canonical little-endian bytes, a point as 0x01 and the 32 bytes
of each affine coordinate; a challenge is 0x00 absorbed, then the 64-byte digest of a COPY of the state reduced modulo the
scalar field.  What goes to the proof stream for a point is the curve's compressed form:
    bn254           x little-endian, bit 6 of the last byte the parity of y (h2_points_decompress_device documents it)
    pallas, vesta   x little-endian, bit 7 of the last byte (bit 255) the parity of y; the identity is 32 zero bytes
Host arithmetic only; the prover and the verifier of the KZG surface and the inner product argument share this class.
Blake2bMidstate is the absorbing side over a state that can be exported (h2_transcript_state_t of the C ABI).
"""
import hashlib

# curve id -> (scalar field prime, base field prime, b of y^2 = x^3 + b)
FIELDS = {
    0: (0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001,
        0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47, 3),
    1: (0x40000000000000000000000000000000224698FC0994A8DD8C46EB2100000001,
        0x40000000000000000000000000000000224698FC094CF91B992D30ED00000001, 5),
    2: (0x40000000000000000000000000000000224698FC094CF91B992D30ED00000001,
        0x40000000000000000000000000000000224698FC0994A8DD8C46EB2100000001, 5),
}
_CURVE_IDS = {"bn254": 0, "pallas": 1, "vesta": 2}


class TranscriptError(ValueError):
    pass


def curve_id(curve):
    return _CURVE_IDS[curve] if isinstance(curve, str) else int(curve)


def sqrt_mod(a, q):
    """a square root of a modulo the prime q, or None (Tonelli-Shanks; q = 3 mod 4 by one power)"""
    a %= q
    if a == 0:
        return 0
    if pow(a, (q - 1) // 2, q) != 1:
        return None
    if q % 4 == 3:
        return pow(a, (q + 1) // 4, q)
    s, t = 0, q - 1
    while t % 2 == 0:
        s, t = s + 1, t // 2
    z = 2
    while pow(z, (q - 1) // 2, q) == 1:
        z += 1
    m, c, x, b = s, pow(z, t, q), pow(a, (t + 1) // 2, q), pow(a, t, q)
    while b != 1:
        i, w = 0, b
        while w != 1:
            w, i = w * w % q, i + 1
        g = pow(c, 1 << (m - i - 1), q)
        m, c, x, b = i, g * g % q, x * g % q, b * g * g % q
    return x


def compress(cid, pt):
    """affine (x, y) canonical ints or None (the identity) -> the 32 bytes of the proof stream"""
    x, y = pt if pt is not None else (0, 0)
    enc = bytearray(x.to_bytes(32, "little"))
    enc[31] |= (y & 1) << (6 if cid == 0 else 7)
    return bytes(enc)


def decompress(cid, data):
    """the inverse of compress: -> (x, y) or None for the identity's bytes; TranscriptError for anything else invalid"""
    _, q, b = FIELDS[cid]
    raw = bytearray(data)
    if cid == 0:
        sign, inf = (raw[31] >> 6) & 1, (raw[31] >> 7) & 1
        raw[31] &= 0x3F
    else:
        sign, inf = (raw[31] >> 7) & 1, 0
        raw[31] &= 0x7F
    x = int.from_bytes(raw, "little")
    if x >= q:
        raise TranscriptError("point x not canonical")
    if inf or (x == 0 and sign == 0):
        return None
    y = sqrt_mod(x * x * x + b, q)
    if y is None:
        raise TranscriptError("point not on the curve")
    if (y & 1) != sign:
        y = q - y
    return (x, y)


class Blake2bTranscript:
    """Blake2bWrite / Blake2bRead with Challenge255.  Writing: `bytes` collects the proof.  Reading: pass the proof."""

    def __init__(self, curve="bn254", proof=None):
        self.curve = curve_id(curve)
        self.p, self.q, _ = FIELDS[self.curve]
        self.state = hashlib.blake2b(digest_size=64, person=b"Halo2-Transcript")
        self.bytes = bytearray()
        self.buf, self.pos = (bytes(proof), 0) if proof is not None else (None, 0)

    # ---- absorbing ------------------------------------------------------------------------------------------
    def common_scalar(self, s):
        self.state.update(b"\x02" + int(s % self.p).to_bytes(32, "little"))

    def common_point(self, pt):
        x, y = pt if pt is not None else (0, 0)
        self.state.update(b"\x01" + x.to_bytes(32, "little") + y.to_bytes(32, "little"))

    def squeeze_challenge(self):
        self.state.update(b"\x00")
        return int.from_bytes(self.state.copy().digest(), "little") % self.p

    # ---- the prover's side ----------------------------------------------------------------------------------
    def write_scalar(self, s):
        self.common_scalar(s)
        self.bytes += int(s % self.p).to_bytes(32, "little")

    def write_point(self, pt):
        self.common_point(pt)
        self.bytes += compress(self.curve, pt)

    # ---- the verifier's side --------------------------------------------------------------------------------
    def _take(self):
        if self.buf is None or self.pos + 32 > len(self.buf):
            raise TranscriptError("proof too short")
        chunk = self.buf[self.pos:self.pos + 32]
        self.pos += 32
        return chunk

    def read_scalar(self):
        v = int.from_bytes(self._take(), "little")
        if v >= self.p:
            raise TranscriptError("scalar not canonical")
        self.common_scalar(v)
        return v

    def read_point(self):
        pt = decompress(self.curve, self._take())
        self.common_point(pt)
        return pt

    def read_point_decoded(self, pt, status=0):
        """read_point for a point whose 32 bytes were decompressed elsewhere (ipa.verify_proofs: one kernel launch for a whole
        batch): consumes the bytes and absorbs `pt`.  status: the decompression's (0 a point, 2 the identity with pt None,
        1 / 3 what read_point refuses: TranscriptError with the bytes consumed, as read_point leaves it)."""
        self._take()
        if status in (1, 3):
            raise TranscriptError("point x not canonical" if status == 1 else "point not on the curve")
        self.common_point(pt)
        return pt


STATE_BYTES = 208                                   # sizeof(h2_transcript_state_t)


class Blake2bMidstate:
    """Blake2bTranscript's absorbing side over an EXPORTABLE state (include/h2hip.h: h2_transcript_state_t), for callers that
    hand a transcript to the device where it stands -- ipa.verify_proofs_bytes; hashlib cannot export one.  The same
    challenges as Blake2bTranscript for the same sequence of calls; `state` continues an exported midstate.  Host only."""

    def __init__(self, curve="bn254", state=None):
        import ctypes
        from . import lib as _lib
        self.curve = curve_id(curve)
        self.p, self.q, _ = FIELDS[self.curve]
        self._L = _lib.load()
        self._check = _lib.check
        self._st = ctypes.create_string_buffer(STATE_BYTES)
        if state is None:
            self._check(self._L.h2_transcript_init(self._st), "h2_transcript_init")
        else:
            state = bytes(state)
            if len(state) != STATE_BYTES:
                raise ValueError("Blake2bMidstate: a state is %d bytes" % STATE_BYTES)
            self._st.raw = state
        self._rinv = pow(1 << 256, -1, self.p)

    def update(self, data):
        data = bytes(data)
        self._check(self._L.h2_transcript_absorb(self._st, data, len(data)), "h2_transcript_absorb")

    def common_scalar(self, s):
        self.update(b"\x02" + int(s % self.p).to_bytes(32, "little"))

    def common_point(self, pt):
        x, y = pt if pt is not None else (0, 0)
        self.update(b"\x01" + x.to_bytes(32, "little") + y.to_bytes(32, "little"))

    def squeeze_challenge(self):
        import ctypes
        out = (ctypes.c_uint64 * 4)()
        self._check(self._L.h2_transcript_challenge(self.curve, self._st, out), "h2_transcript_challenge")
        return sum(int(out[i]) << (64 * i) for i in range(4)) * self._rinv % self.p

    def export(self):
        """the 208 bytes of the state as it stands"""
        return bytes(self._st.raw)
