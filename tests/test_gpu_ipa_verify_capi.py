"""h2_ipa_replay_device and h2_ipa_verify_proofs on the GPU: the device replay against the host's transcript word for word and
byte for byte, and the batch verifier of the C ABI against ipa.verify_proof item by item and against ipa.verify_proofs --
verdicts, the number of combined checks, all_ok -- for good batches and for every kind of bad item at the first, the last,
two adjacent and all positions.

The replay's status 3 (a challenge u_j = 0) is not tested: producing one means finding a Blake2b preimage of a multiple of
the field's modulus, so no input a test can make reaches that branch."""
import ctypes
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CID = {"pallas": 1, "vesta": 2}
# absorbed lengths in front of the proofs of ONE launch: lanes of a wave compress at different pieces, one starts with a full
# uncompressed buffer (128), one with an empty one
PREFIXES = [0, 1, 62, 63, 64, 127, 128, 129, 300]


def limbs(values):
    buf = b"".join(int(v).to_bytes(32, "little") for v in values)
    return np.frombuffer(buf, dtype=np.uint64).reshape(-1, 4).copy()


class Rng:
    """a deterministic callable n -> n bytes"""

    def __init__(self, seed):
        self.r = random.Random(seed)

    def __call__(self, n):
        return bytes(self.r.getrandbits(8) for _ in range(n))


def prefix_bytes(i):
    n = PREFIXES[i % len(PREFIXES)]
    return bytes(random.Random(0x505246 + i).getrandbits(8) for _ in range(n))


def off_curve_x(q, start):
    """an x in range with no point on the curve"""
    from halo2_prover_amd.transcript import sqrt_mod
    x = start
    while sqrt_mod(x * x * x + 5, q) is not None:
        x += 1
    return x


_POOL = {}


def point_pool(curve):
    """64 points of the curve as (x, y) canonical ints: computed once, shared, never changed"""
    if curve not in _POOL:
        import oracle_lib as O
        from halo2_prover_amd.transcript import FIELDS
        q = FIELDS[CID[curve]][1]
        rinv = pow(1 << 256, -1, q)
        raw = O.synth_bases(CID[curve], 0x5245504C + CID[curve], 64).reshape(64, 8)
        pts = []
        for row in raw:
            x = int.from_bytes(row[:4].tobytes(), "little") * rinv % q
            y = int.from_bytes(row[4:].tobytes(), "little") * rinv % q
            assert (y * y - x * x * x - 5) % q == 0
            pts.append((x, y))
        _POOL[curve] = pts
    return _POOL[curve]


# ------------------------------------------------------------------------------------------------------- the replay ----
def replay_case(h2, curve, k, count):
    """one launch of `count` lanes against the host's replay"""
    import torch
    from halo2_prover_amd.transcript import FIELDS, Blake2bMidstate, Blake2bTranscript, compress
    L = h2.load()
    cid = CID[curve]
    p, q, _ = FIELDS[cid]
    R = (1 << 256) % p
    per = 2 * k + 1
    pool = point_pool(curve)
    rnd = random.Random(0x5245504C4159 + 1000 * k + count)
    wire, scalars, states, want_status, want_out, want_state = bytearray(), bytearray(), bytearray(), [], [], []
    for lane in range(count):
        prefix = prefix_bytes(lane + k)
        pts = [pool[rnd.randrange(64)] for _ in range(per)]
        enc = [compress(cid, pt) for pt in pts]
        c, f = rnd.randrange(p), rnd.randrange(p)
        c_raw, f_raw = c.to_bytes(32, "little"), f.to_bytes(32, "little")
        status = 0
        if lane == 0:                                    # one identity: absorbed as 0x01 and 64 zero bytes
            at = rnd.randrange(per)
            pts[at], enc[at] = None, bytes(32)
        elif lane == 1 and count >= 3:                   # decompression status 1: x not canonical
            enc[rnd.randrange(per)] = (q + 5).to_bytes(32, "little")
            status = 1
        elif lane == 2 and count >= 3:                   # decompression status 3: no such point
            enc[rnd.randrange(per)] = off_curve_x(q, rnd.randrange(q >> 1)).to_bytes(32, "little")
            status = 1
        elif lane == 3 and count >= 65:
            c_raw, status = p.to_bytes(32, "little"), 2
        elif lane == 4 and count >= 65:
            f_raw, status = ((1 << 256) - 1).to_bytes(32, "little"), 2
        wire += b"".join(enc)
        scalars += c_raw + f_raw
        mid = Blake2bMidstate(curve)
        mid.update(prefix)
        states += mid.export()
        want_status.append(status)
        if status:
            want_out.append(None)
            want_state.append(None)
            continue
        # the host's replay, through both classes: the challenges agree and the midstate is what the device must leave
        tr = Blake2bTranscript(curve)
        tr.state.update(prefix)
        row = []
        for t in (tr, mid):
            got = []
            t.common_point(pts[0])
            got += [t.squeeze_challenge(), t.squeeze_challenge()]
            for j in range(k):
                t.common_point(pts[1 + 2 * j])
                t.common_point(pts[2 + 2 * j])
                got.append(t.squeeze_challenge())
            t.common_scalar(c)
            t.common_scalar(f)
            row.append(got + [c, f])
        assert row[0] == row[1]
        want_out.append(limbs([x * R % p for x in row[0]]))
        want_state.append(mid.export())
    G = count * per
    d_wire = torch.from_numpy(np.frombuffer(bytes(wire), dtype=np.int64).copy()).cuda()
    d_points = torch.zeros((G, 8), dtype=torch.int64, device="cuda")
    d_pstatus = torch.empty(G, dtype=torch.uint8, device="cuda")
    h2.pasta_points_decompress_device(d_wire.data_ptr(), G, d_points.data_ptr(), d_pstatus.data_ptr(), curve=curve)
    d_states = torch.from_numpy(np.frombuffer(bytes(states), dtype=np.int64).copy()).cuda()
    d_scalars = torch.from_numpy(np.frombuffer(bytes(scalars), dtype=np.int64).copy()).cuda()
    d_out = torch.full((count * (k + 4) + 1, 4), -1, dtype=torch.int64, device="cuda")
    d_status = torch.full((count + 16,), 0xEE, dtype=torch.uint8, device="cuda")
    d_states_out = torch.full((count * 26 + 2,), -1, dtype=torch.int64, device="cuda")
    st = L.h2_ipa_replay_device(cid, k, count, d_states.data_ptr(), d_points.data_ptr(), d_pstatus.data_ptr(), d_scalars.data_ptr(),
                                d_out.data_ptr(), d_status.data_ptr(), d_states_out.data_ptr(), None)
    assert st == 0
    torch.cuda.synchronize()
    status = d_status.cpu().numpy()
    assert list(status[:count]) == want_status and (status[count:] == 0xEE).all()
    out = d_out.cpu().numpy().view(np.uint64)
    so = d_states_out.cpu().numpy()
    assert (out[count * (k + 4)] == np.uint64(0xFFFFFFFFFFFFFFFF)).all() and (so[count * 26:] == -1).all()    # nothing behind the rows
    for lane in range(count):
        if want_status[lane]:
            continue                                     # the row of a refused proof is unspecified; its neighbours' are not
        assert (out[lane * (k + 4):(lane + 1) * (k + 4)] == want_out[lane]).all(), (curve, k, count, lane)
        assert so[lane * 26:(lane + 1) * 26].tobytes() == want_state[lane], (curve, k, count, lane)
    # without d_states_out: the same rows
    d_out2 = torch.zeros_like(d_out)
    st = L.h2_ipa_replay_device(cid, k, count, d_states.data_ptr(), d_points.data_ptr(), d_pstatus.data_ptr(), d_scalars.data_ptr(),
                                d_out2.data_ptr(), d_status.data_ptr(), None, None)
    assert st == 0
    torch.cuda.synchronize()
    out2 = d_out2.cpu().numpy().view(np.uint64)
    for lane in range(count):
        if not want_status[lane]:
            assert (out2[lane * (k + 4):(lane + 1) * (k + 4)] == want_out[lane]).all()


@pytest.mark.parametrize("k", [1, 2, 3, 5])
@pytest.mark.parametrize("curve", ["pallas", "vesta"])
def test_replay_matches_the_host(h2, curve, k):
    for count in (1, 3, 65, 130):                        # one lane, a ragged wave, more than one wave, a ragged last one
        replay_case(h2, curve, k, count)


def test_replay_argument_checks(h2):
    import torch
    L = h2.load()
    fn = L.h2_ipa_replay_device
    buf = torch.zeros(4096, dtype=torch.int64, device="cuda")
    a = [buf.data_ptr() + 1024 * i for i in range(7)]    # states, points, point status, scalars, out, status, states out
    assert fn(1, 2, 0, None, None, None, None, None, None, None, None) == 0          # count = 0
    assert fn(0, 2, 1, *a, None) == -1                                               # BN254: the wire form is the Pasta one
    assert fn(3, 2, 1, *a, None) == -1                                               # unknown curve
    assert fn(1, 0, 1, *a, None) == -1                                               # k = 0
    assert fn(1, 21, 1, *a, None) == -1                                              # k > H2_IPA_MAX_K
    for i in range(6):                                                               # a null pointer
        b = list(a)
        b[i] = None
        assert fn(1, 2, 1, *b, None) == -1, i
    for i in (0, 1, 3, 4, 6):                                                        # not 16-byte aligned
        b = list(a)
        b[i] += 8
        assert fn(1, 2, 1, *b, None) == -1, i
    torch.cuda.synchronize()
    assert not buf.cpu().numpy().any()                                               # a refused call has enqueued nothing


# ----------------------------------------------------------------------------------------------------- the verdicts ----
_BATCH = {}
SPECIAL = 9                                          # the proof of the zero polynomial under the identity


def batch(curve, k):
    """params, nine proofs from ONE ipa.create_proofs call -- each of its own polynomial, blind, point and transcript prefix --
    and a tenth for the commitment that is the identity: shared by the tests, never changed"""
    key = (curve, k)
    if key in _BATCH:
        return _BATCH[key]
    import halo2_prover_amd as h2
    import oracle_lib as O
    from halo2_prover_amd import ipa
    h2.init(0)
    cid, n = CID[curve], 1 << k
    pts = O.synth_bases(cid, 0x49564200 + 16 * k + cid, n + 2).reshape(n + 2, 8)
    params = ipa.ParamsIPA(curve, k, pts[:n], pts[n + 1], pts[n])
    p = params.p
    R = (1 << 256) % p
    entries, items = [], []
    for i in range(SPECIAL + 1):
        rnd = random.Random(0xCA910 + 64 * k + i)
        poly = [rnd.randrange(p) for _ in range(n)] if i != SPECIAL else [0] * n
        blind, x3 = (rnd.randrange(p) if i != SPECIAL else 0), rnd.randrange(1, p)
        poly_m = limbs([c * R % p for c in poly])
        v = sum(c * pow(x3, j, p) for j, c in enumerate(poly)) % p
        prefix = prefix_bytes(i) if i != SPECIAL else b"in front of the identity's proof"
        tr = h2.Blake2bTranscript(curve)
        tr.state.update(prefix)
        entries.append(dict(P=params.commit(poly_m, blind), x3=x3, v=v, prefix=prefix))
        items.append((tr, poly_m, blind, x3, Rng(300 + i), None))
    for e, proof in zip(entries, ipa.create_proofs(params, items)):
        e["proof"] = proof
    assert entries[SPECIAL]["P"] is None and len(entries[0]["proof"]) == 32 * (2 * k + 3)
    _BATCH[key] = dict(curve=curve, k=k, params=params, entries=entries)
    return _BATCH[key]


def flip(proof, byte, bit=0):
    out = bytearray(proof)
    out[byte] ^= 1 << bit
    return bytes(out)


KINDS = ["bit of L_j", "bit of c", "bit of f", "wrong v", "wrong P", "P the identity", "one word short", "x off the curve"]


def spoil(B, e, kind, other):
    k, params = B["k"], B["params"]
    e = dict(e)
    proof = e["proof"]
    lj = 32 * (1 + 2 * (k - 1))                          # L_(k-1)
    if kind == "bit of L_j":
        e["proof"] = flip(proof, lj + 5, 3)
    elif kind == "bit of c":
        e["proof"] = flip(proof, 32 * (2 * k + 1) + 3, 2)
    elif kind == "bit of f":
        e["proof"] = flip(proof, 32 * (2 * k + 2) + 9, 6)
    elif kind == "wrong v":
        e["v"] = (e["v"] + 1) % params.p
    elif kind == "wrong P":
        e["P"] = other["P"]
    elif kind == "P the identity":                       # the proof made for it, behind this item's own prefix: a good item
        e = dict(B["entries"][SPECIAL])
    elif kind == "one word short":
        e["proof"] = proof[:-32]
    else:
        x = off_curve_x(params.q, int.from_bytes(proof[lj:lj + 31], "little"))
        e["proof"] = proof[:lj] + x.to_bytes(32, "little") + proof[lj + 32:]
    return e


def verdicts(B, entries, seed=5):
    """the three routes on the same batch -> (the C ABI's, verify_proof's item by item, verify_proofs', both stats)"""
    import halo2_prover_amd as h2
    from halo2_prover_amd import ipa
    curve, params = B["curve"], B["params"]

    def reading(e):
        tr = h2.Blake2bTranscript(curve, e["proof"])
        tr.state.update(e["prefix"])
        return tr

    def midstate(e, as_bytes):
        mid = h2.Blake2bMidstate(curve)
        mid.update(e["prefix"])
        return mid.export() if as_bytes else mid
    single = [ipa.verify_proof(params, reading(e), e["P"], e["x3"], e["v"]) for e in entries]
    ref_stats, stats = {}, {}
    ref = ipa.verify_proofs(params, [(reading(e), e["P"], e["x3"], e["v"]) for e in entries], rng=Rng(seed), stats=ref_stats)
    got = ipa.verify_proofs_bytes(params, [(midstate(e, i & 1), e["proof"], e["P"], e["x3"], e["v"]) for i, e in enumerate(entries)],
                                  rng=Rng(seed), stats=stats)
    return got, single, ref, stats, ref_stats


@pytest.mark.parametrize("k", [2, 3, 5])
@pytest.mark.parametrize("curve", ["pallas", "vesta"])
def test_verdicts_match_verify_proof(h2, curve, k):
    B = batch(curve, k)
    used = set()
    for N in (1, 2, 5, 9):
        good = B["entries"][:N]
        patterns = [set(), {0}, {N - 1}, {N // 2, min(N // 2 + 1, N - 1)}, set(range(N))]      # none, first, last, adjacent, all
        for t, bad in enumerate(patterns):
            entries = []
            for i, e in enumerate(good):
                if i in bad:
                    kind = KINDS[(i + 3 * t + N) % len(KINDS)]
                    used.add(kind)
                    e = spoil(B, e, kind, B["entries"][(i + 1) % SPECIAL])
                entries.append(e)
            got, single, ref, stats, ref_stats = verdicts(B, entries, seed=7 * N + t)
            assert got == single == ref, (curve, k, N, sorted(bad))
            assert stats["checks"] == ref_stats["checks"], (curve, k, N, sorted(bad))          # the same halving, the same draws
            assert stats["all_ok"] == all(got)
            if not bad:
                assert got == [True] * N and stats["checks"] == 1
    assert used == set(KINDS)                              # every kind of culprit has been in a batch


@pytest.mark.parametrize("curve", ["pallas", "vesta"])
def test_every_kind_alone_and_among_good_items(h2, curve):
    B = batch(curve, 3)
    good = B["entries"][:5]
    for kind in KINDS:
        bad = spoil(B, good[2], kind, good[3])
        want = kind == "P the identity"
        for entries in ([bad], good[:2] + [bad] + good[3:]):
            got, single, ref, stats, ref_stats = verdicts(B, entries)
            assert got == single == ref and got[len(entries) // 2] == want, kind
            assert got.count(False) == (0 if want else 1) and stats["checks"] == ref_stats["checks"], kind


def test_repeat_on_one_context(h2):
    """one call after another with a different N: the arenas are released and taken again"""
    B = batch("pallas", 3)
    e = B["entries"]
    nine = e[:4] + [spoil(B, e[4], "wrong v", e[5])] + e[5:9]
    want9 = [i != 4 for i in range(9)]
    for entries, want in ((nine, want9), (e[:2], [True, True]), (nine, want9), (e[:1], [True]), (nine, want9)):
        got, single, ref, _, _ = verdicts(B, entries)
        assert got == single == ref == want


def test_verify_proofs_argument_checks(h2):
    from halo2_prover_amd import ipa
    import oracle_lib as O
    B = batch("pallas", 2)
    params, e = B["params"], B["entries"][0]
    L = h2.load()
    assert ipa.verify_proofs_bytes(params, []) == []
    all_ok, checks = ctypes.c_int(-1), ctypes.c_size_t(99)
    fn = L.h2_ipa_verify_proofs
    tail = (None, None, None, ctypes.byref(all_ok), ctypes.byref(checks))
    assert fn(1, params.bases.handle, 2, 0, None, None, None, None, None, None, *tail) == 0
    assert (all_ok.value, checks.value) == (1, 0)                                    # count = 0: nothing to refuse
    assert fn(0, params.bases.handle, 2, 0, None, None, None, None, None, None, *tail) == -1     # BN254
    assert fn(1, params.bases.handle, 0, 0, None, None, None, None, None, None, *tail) == -1     # k = 0
    assert fn(1, params.bases.handle, 3, 0, None, None, None, None, None, None, *tail) == -1     # not 2^k + 2 bases
    assert fn(1, 0xDEAD, 2, 0, None, None, None, None, None, None, *tail) == -4                  # no such handle
    assert fn(1, params.bases.handle, 2, 1, None, None, None, None, None, None, *tail) == -1     # null arrays with count > 0
    with pytest.raises(ValueError):
        ipa.verify_proofs_bytes(params, [(b"short", e["proof"], e["P"], e["x3"], e["v"])])
    pts = O.synth_bases(0, 0x49564201, 6).reshape(6, 8)
    with pytest.raises(ValueError):
        ipa.verify_proofs_bytes(ipa.ParamsIPA("bn254", 2, pts[:4], pts[5], pts[4]), [])
